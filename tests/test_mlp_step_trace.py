"""Which primitives each step form of the whole-step trainer calls, with which arguments, in which order (CPU only, no kernel runs).

csrc/tnn_mlp.cpp is host-only C++ on top of the C ABI, so it compiles against logging stubs generated from include/tnn_hip.h:
every `int` entry point the trainer does not define itself prints its name and arguments and returns 0.  Pointers print as
A<k>+<byte offset> (k-th allocation of the process: x, y and loss_out are A1..A3, tnn_mlp_create's follow), 0, or `host`;
doubles as %.17g.  One process per case (TNN_DP_XCHG and TNN_BUCKET_BYTES are read once per process); the concatenated output
is compared with tests/golden/mlp_step_traces.txt, recorded from the trainer source BEFORE its step forms were restructured:

    python tests/test_mlp_step_trace.py --record [--source path/to/an/older/tnn_mlp.cpp]

rewrites the fixture (from the given source; default: the tree's), without --record it prints the traces.
"""

import difflib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tnn_hip.h")
SOURCE = os.path.join(ROOT, "tinynn-autograd_amd", "csrc", "tnn_mlp.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "mlp_step_traces.txt")

PROLOGUE = r"""
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>
#include "tnn_hip.h"

static struct { int world = 1, rank = 0, p2p = 0, head_fits = 0, head_bwd_fits = 0, xchg_fits = 0; long fail_at = -1; } g_case;
static long g_calls = 0;            // primitive calls so far (fail_at counts them from the first entry point after create)
static bool g_quiet = false;
static const uint64_t kFirst = 256; // fake device addresses k << 40 lie above any user-space address; never dereferenced
static uint64_t g_next = kFirst;

static const char* P(const void* p) {
    static char ring[64][40];
    static int i = 0;
    const uint64_t a = (uint64_t)p, k = a >> 40;
    if (!a) return "0";
    if (k < kFirst || k >= g_next) return "host";
    char* b = ring[i++ & 63];
    snprintf(b, 40, "A%llu+%llu", (unsigned long long)(k - kFirst + 1), (unsigned long long)(a & ((1ull << 40) - 1)));
    return b;
}
static void* fake_alloc() { return (void*)(g_next++ << 40); }
// one line per primitive call; the fail_at-th call fails
static int emit(const char* fmt, ...) {
    if (!g_quiet) {
        va_list ap;
        va_start(ap, fmt);
        vprintf(fmt, ap);
        va_end(ap);
        putchar('\n');
    }
    if (g_calls++ == g_case.fail_at) { puts("  ^ returns 1"); return 1; }
    return 0;
}
namespace tnn {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("error: ");
    vprintf(fmt, ap);
    va_end(ap);
    putchar('\n');
}
}
extern "C" {
int tnn_malloc(size_t bytes, void** out) { *out = fake_alloc(); return emit("tnn_malloc %zu -> %s", bytes, P(*out)); }
int tnn_free(void* p) { return emit("tnn_free %s", P(p)); }
int tnn_mlp_head_fits(int64_t rows, int64_t n_hidden, int64_t n_classes, int dtype, int* fits) {
    *fits = g_case.head_fits;
    return emit("tnn_mlp_head_fits %lld %lld %lld %d -> %d", (long long)rows, (long long)n_hidden, (long long)n_classes, dtype, *fits);
}
int tnn_mlp_head_bwd_fits(int64_t rows, int64_t n_in, int64_t n_hidden, int64_t n_classes, int dtype, int* fits) {
    *fits = g_case.head_bwd_fits;
    return emit("tnn_mlp_head_bwd_fits %lld %lld %lld %lld %d -> %d", (long long)rows, (long long)n_in, (long long)n_hidden,
                (long long)n_classes, dtype, *fits);
}
int tnn_mlp_head_bwd_xchg_fits(int64_t rows, int64_t n_in, int64_t n_hidden, int64_t n_classes, int dtype, int* fits) {
    *fits = g_case.xchg_fits;
    return emit("tnn_mlp_head_bwd_xchg_fits %lld %lld %lld %lld %d -> %d", (long long)rows, (long long)n_in, (long long)n_hidden,
                (long long)n_classes, dtype, *fits);
}
int tnn_comm_world(int* rank, int* world) {
    *rank = g_case.rank;
    *world = g_case.world;
    return emit("tnn_comm_world -> %d %d", *rank, *world);
}
int tnn_p2p_status(int* connected, int* enabled, int* dead) {
    if (connected) *connected = g_case.p2p;
    if (enabled) *enabled = g_case.p2p;
    if (dead) *dead = 0;
    return emit("tnn_p2p_status -> %d", g_case.p2p);
}
int tnn_bias_bf16_adam_multi(int n_layers, const void* const* dz, int64_t rows, const int64_t* cols, void* const* db_f32,
                             void* const* p_master, void* const* m, void* const* v, void* const* w_bf16, double lr, double b1,
                             double b2, double eps, const void* pows_f64) {
    std::string s = "tnn_bias_bf16_adam_multi " + std::to_string(n_layers) + " rows " + std::to_string((long long)rows);
    for (int l = 0; l < n_layers; ++l) {
        s += std::string(" [") + P(dz[l]) + " " + std::to_string((long long)cols[l]);
        for (void* const* a : {db_f32, p_master, m, v, w_bf16}) s += std::string(" ") + P(a[l]);
        s += "]";
    }
    return emit("%s %.17g %.17g %.17g %.17g %s", s.c_str(), lr, b1, b2, eps, P(pows_f64));
}
"""

MAIN = r"""
static std::map<std::string, std::string> g_arg;
static long arg(const char* key, long dflt) { return g_arg.count(key) ? atol(g_arg[key].c_str()) : dflt; }
static std::vector<std::string> split(const std::string& s) {
    std::vector<std::string> out;
    size_t at = 0;
    while (at <= s.size() && !s.empty()) {
        size_t comma = s.find(',', at);
        if (comma == std::string::npos) comma = s.size();
        out.push_back(s.substr(at, comma - at));
        at = comma + 1;
    }
    return out;
}

// one case: key=value arguments (see CASES in tests/test_mlp_step_trace.py)
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        g_arg[std::string(argv[i], eq - argv[i])] = eq + 1;
    }
    std::vector<int64_t> w;
    for (const std::string& s : split(g_arg["w"])) w.push_back(atoll(s.c_str()));
    const std::string dt = g_arg.count("dtype") ? g_arg["dtype"] : "f32";
    const int dtype = dt == "f64" ? TNN_F64 : dt == "bf16" ? TNN_BF16 : dt == "i64" ? TNN_I64 : TNN_F32;
    const int64_t max_rows = arg("max_rows", 128), rows = arg("rows", max_rows);
    g_case.world = (int)arg("world", 1);
    g_case.rank = (int)arg("rank", 0);
    g_case.p2p = (int)arg("p2p", 0);
    g_case.head_fits = (int)arg("head_fits", 0);
    g_case.head_bwd_fits = (int)arg("head_bwd_fits", 0);
    g_case.xchg_fits = (int)arg("xchg_fits", 0);
    void *x = fake_alloc(), *y = fake_alloc(), *loss_out = fake_alloc();
    if (!arg("loss_out", 1)) loss_out = nullptr;
    const bool trace_create = arg("trace_create", 0) != 0;
    void* h = nullptr;
    g_quiet = !trace_create;
    int rc = tnn_mlp_create((int)w.size() - 1, w.data(), max_rows, (int)arg("loss", 0), (int)arg("opt", 1), 1e-3, 0.9, 0.999, 1e-8,
                            dtype, &h);
    g_quiet = false;
    if (trace_create || rc) printf("tnn_mlp_create rc=%d\n", rc);
    if (rc) return 0;
    if (!arg("keep", 1)) tnn_mlp_keep_grads(h, 0);
    int win_first = -1, win_count = -1;
    if (g_arg.count("win")) {
        sscanf(g_arg["win"].c_str(), "%d,%d", &win_first, &win_count);
        tnn_mlp_launch_window(h, win_first, win_count, nullptr);
    }
    g_calls = 0;
    g_case.fail_at = arg("fail_at", -1);
    for (const std::string& op : split(g_arg["ops"])) {
        printf("-- %s\n", op.c_str());
        if (op.rfind("world:", 0) == 0) { g_case.world = atoi(op.c_str() + 6); continue; }
        if (op == "step") rc = tnn_mlp_step(h, x, y, rows, loss_out);
        else if (op == "sharded") rc = tnn_mlp_step_sharded(h, x, y, rows, loss_out);
        else if (op == "forward") rc = tnn_mlp_forward(h, x, rows, loss_out);
        else if (op == "forward_stats") rc = tnn_mlp_forward_stats(h, x, rows, nullptr);
        else if (op == "backward") rc = tnn_mlp_backward(h, x, y, rows, rows, nullptr, loss_out);
        else if (op == "update") rc = tnn_mlp_update(h);
        else if (op == "sync") rc = tnn_mlp_sync_params(h);
        else if (op == "gather") rc = tnn_mlp_gather_masters(h);
        else if (op == "bf16_weights") { void* w16 = nullptr; rc = tnn_mlp_bf16_weights(h, &w16); }
        else if (op == "masters") { int mw = -1; rc = tnn_mlp_masters_sharded(h, &mw); printf("masters_world=%d\n", mw); }
        else { fprintf(stderr, "unknown op %s\n", op.c_str()); return 2; }
        printf("rc=%d", rc);
        if (op == "step") {         // (the value after tnn_mlp_step_sharded is not part of the header's contract)
            int n = -1;
            tnn_mlp_launch_window(h, 0, -1, &n);
            if (win_first >= 0) tnn_mlp_launch_window(h, win_first, win_count, nullptr);
            printf(" calls_in_last_step=%d", n);
        }
        putchar('\n');
    }
    g_case.fail_at = -1;
    g_quiet = !trace_create;
    rc = tnn_mlp_destroy(h);
    if (trace_create) printf("tnn_mlp_destroy rc=%d\n", rc);
    return 0;
}
"""


def declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return re.findall(r"TNN_API\s+([\w\s\*]+?)\b(tnn_\w+)\s*\(([^)]*)\)\s*;", text)


def stub(name, params):
    """`int name(params) { return emit("name %lld ...", ...); }`"""
    fmt, vals = [name], []
    for n, p in enumerate(params):
        p = " ".join(p.split())
        ctype = re.sub(r"\b\w+$", "", p).strip()
        a = "a%d" % n
        params[n] = "%s %s" % (ctype, a)
        if "*" in ctype:
            fmt.append("%s"); vals.append("P((const void*)%s)" % a)
        elif ctype == "double":
            fmt.append("%.17g"); vals.append(a)
        else:
            assert ctype in ("int", "int64_t", "size_t"), (name, p)
            fmt.append("%lld"); vals.append("(long long)%s" % a)
    return 'int %s(%s) { return emit(%s); }\n' % (name, ", ".join(params), ", ".join(['"%s"' % " ".join(fmt)] + vals))


def harness_source(trainer_source):
    own = set(re.findall(r"^int (tnn_\w+)\(", open(trainer_source).read(), flags=re.M))
    hand_written = set(re.findall(r"^int (tnn_\w+)\(", PROLOGUE, flags=re.M))
    out = [PROLOGUE]
    for ret, name, params in declarations():
        if ret.strip() != "int" or name in own or name in hand_written:
            continue
        params = [] if params.strip() in ("", "void") else params.split(",")
        out.append(stub(name, params))
    out.append('}  // extern "C"\n#include "%s"\n' % os.path.abspath(trainer_source))
    out.append(MAIN)
    return "".join(out)


def build_harness(workdir, trainer_source=SOURCE, extra_flags=()):
    src = os.path.join(str(workdir), "mlp_trace.cpp")
    exe = os.path.join(str(workdir), "mlp_trace")
    with open(src, "w") as f:
        f.write(harness_source(trainer_source))
    subprocess.check_call(["g++", "-std=c++17", "-O0", *extra_flags, "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    return exe


MNIST = "784,256,128,10"
DEEP = "784,208,112,80,32,10"           # a generic merged head (80 -> 32 -> 10)
GENERIC3 = "96,80,32,10"
TUNED3 = "96,64,128,10"
BIG = "2048,2048,16"                    # >= 2^22 parameters
B16 = "64,64,64"


def _merged_sharded_cases():
    out = []
    shapes = [("128rows_tuned", "w=%s max_rows=128" % MNIST), ("256rows_tuned", "w=%s max_rows=256" % MNIST),
              ("256rows_generic", "w=%s max_rows=256" % GENERIC3), ("300rows_tuned", "w=%s max_rows=512 rows=300" % TUNED3)]
    modes = [("p2p_xchg", "p2p=1 xchg_fits=1", {}), ("p2p_noxchgfit", "p2p=1 xchg_fits=0", {}),
             ("p2p_dpxchg0", "p2p=1 xchg_fits=1", {"TNN_DP_XCHG": "0"}), ("rccl", "p2p=0", {})]
    for sname, shape in shapes:
        for mname, mode, env in modes:
            out.append(("sharded_merged_%s_%s_w2" % (sname, mname), "%s world=2 rank=1 %s ops=sharded" % (shape, mode), env))
    out.append(("sharded_merged_128rows_tuned_p2p_xchg_w1", "w=%s max_rows=128 world=1 p2p=1 xchg_fits=1 ops=sharded,sharded" % MNIST, {}))
    out.append(("sharded_merged_128rows_generic_p2p_xchg_w2", "w=%s max_rows=128 world=2 rank=1 p2p=1 xchg_fits=1 ops=sharded" % GENERIC3, {}))
    out.append(("sharded_merged_256rows_tuned_rccl_w1", "w=%s max_rows=256 world=1 ops=sharded" % MNIST, {}))
    out.append(("sharded_merged_256rows_generic_p2p_w1", "w=%s max_rows=256 world=1 p2p=1 xchg_fits=1 ops=sharded" % GENERIC3, {}))
    return out


# (name, arguments of the harness, environment of the child)
CASES = [
    # ---- tnn_mlp_create / _destroy: the allocation sizes and their order
    ("create_f32_mnist", "w=%s max_rows=256 trace_create=1 ops=" % MNIST, {}),
    ("create_f32_mse_1layer", "w=20,5 max_rows=8 loss=1 trace_create=1 ops=", {}),
    ("create_f64", "w=20,12,5 max_rows=8 dtype=f64 trace_create=1 ops=", {}),
    ("create_bf16", "w=%s max_rows=64 loss=1 dtype=bf16 trace_create=1 ops=" % B16, {}),
    ("create_bad_width", "w=20,0,5 max_rows=8 ops=", {}),
    ("create_bad_dtype", "w=20,5 max_rows=8 dtype=i64 ops=", {}),
    # ---- tnn_mlp_step, fp32, softmax + Adam
    ("step_mnist_128", "w=%s max_rows=128 head_fits=1 ops=step,step" % MNIST, {}),
    ("step_mnist_32", "w=%s max_rows=128 rows=32 head_fits=1 ops=step" % MNIST, {}),
    ("step_mnist_128_no_loss_out_drop_grads", "w=%s max_rows=128 head_fits=1 loss_out=0 keep=0 ops=step" % MNIST, {}),
    ("step_deep_generic_head", "w=%s max_rows=128 head_fits=0 head_bwd_fits=1 ops=step" % DEEP, {}),
    ("step_unmerged_2layer", "w=784,128,10 max_rows=128 head_fits=1 ops=step", {}),
    ("step_unmerged_250", "w=784,250,128,10 max_rows=128 head_fits=1 ops=step", {}),
    ("step_rowblocks_256_tuned", "w=%s max_rows=256 ops=step" % MNIST, {}),
    ("step_rowblocks_300_tuned", "w=%s max_rows=512 rows=300 ops=step" % MNIST, {}),
    ("step_rowblocks_256_generic", "w=%s max_rows=256 ops=step" % DEEP, {}),
    ("step_rowblocks_300_generic", "w=%s max_rows=512 rows=300 ops=step" % DEEP, {}),
    ("step_rowblocks_1024_and_past", "w=%s max_rows=1100 rows=1024 ops=step" % MNIST, {}),
    ("step_past_rowblocks_1025", "w=%s max_rows=1100 rows=1025 ops=step" % MNIST, {}),
    ("step_rowblocks_hidden_not_16", "w=784,250,128,10 max_rows=256 ops=step", {}),
    ("step_one_workgroup_16_classes", "w=784,64,10 max_rows=128 ops=step", {}),
    ("step_one_workgroup_wide_head", "w=784,64,100 max_rows=32 ops=step", {}),
    ("step_one_workgroup_1layer", "w=784,10 max_rows=128 loss_out=0 ops=step", {}),
    ("step_fallback_wide_head", "w=784,64,100 max_rows=64 ops=step", {}),
    ("step_fallback_sgd", "w=784,64,10 max_rows=128 opt=0 ops=step", {}),
    ("step_fallback_sgd_1layer", "w=784,10 max_rows=128 opt=0 loss_out=0 ops=step", {}),
    ("step_fallback_momentum", "w=784,64,10 max_rows=128 opt=2 ops=step", {}),
    ("step_fallback_f64", "w=784,64,100 max_rows=32 dtype=f64 ops=step", {}),
    ("step_one_workgroup_f64", "w=784,64,10 max_rows=128 dtype=f64 ops=step", {}),
    ("step_mse", "w=784,64,10 max_rows=128 loss=1 ops=step", {}),
    ("step_mse_sgd_no_loss_out", "w=784,64,10 max_rows=128 loss=1 opt=0 loss_out=0 ops=step", {}),
    ("step_big_softmax_drop_grads", "w=%s max_rows=128 keep=0 ops=step" % BIG, {}),
    ("step_big_softmax_drop_grads_no_loss_out", "w=%s max_rows=128 keep=0 loss_out=0 ops=step" % BIG, {}),
    ("step_big_mse_drop_grads", "w=%s max_rows=128 loss=1 keep=0 ops=step" % BIG, {}),
    ("step_big_keep_grads", "w=%s max_rows=128 keep=1 ops=step" % BIG, {}),
    ("step_mnist_window_1_2", "w=%s max_rows=128 head_fits=1 win=1,1 ops=step,step" % MNIST, {}),
    ("step_rowblocks_window_1_2", "w=%s max_rows=256 win=1,2 ops=step" % DEEP, {}),
    ("step_rows_out_of_range", "w=%s max_rows=128 rows=129 ops=step,sharded,forward,forward_stats,backward" % MNIST, {}),
    # ---- tnn_mlp_step, bf16 (MSE + Adam)
    ("step_bf16_fused", "w=%s max_rows=64 loss=1 dtype=bf16 keep=0 ops=step,bf16_weights,sync,bf16_weights" % B16, {}),
    ("step_bf16_ct", "w=%s max_rows=64 loss=1 dtype=bf16 keep=0 ops=step" % B16, {"TNN_E_STEP": "ct"}),
    ("step_bf16_long", "w=%s max_rows=64 loss=1 dtype=bf16 keep=0 ops=step,bf16_weights" % B16, {"TNN_E_STEP": "long"}),
    ("step_bf16_32rows", "w=%s max_rows=64 rows=32 loss=1 dtype=bf16 keep=0 loss_out=0 ops=step" % B16, {}),
    ("step_bf16_3layer_fused", "w=64,128,64,64 max_rows=128 loss=1 dtype=bf16 keep=0 ops=step", {}),
    ("step_bf16_keep_grads", "w=%s max_rows=64 loss=1 dtype=bf16 keep=1 ops=step" % B16, {}),
    ("step_bf16_softmax_is_an_error", "w=%s max_rows=64 loss=0 dtype=bf16 ops=backward" % B16, {}),
    ("step_bf16_sgd_is_an_error", "w=%s max_rows=64 loss=1 opt=0 dtype=bf16 ops=update" % B16, {}),
    # ---- tnn_mlp_step_sharded
    *_merged_sharded_cases(),
    ("sharded_one_workgroup_p2p", "w=784,64,10 max_rows=128 world=2 rank=1 p2p=1 ops=sharded", {}),
    ("sharded_general_adam", "w=784,64,10 max_rows=128 world=2 rank=1 ops=sharded,sharded", {}),
    ("sharded_general_adam_w1", "w=784,64,10 max_rows=128 world=1 ops=sharded", {}),
    ("sharded_general_sgd", "w=784,64,10 max_rows=128 opt=0 world=2 rank=1 p2p=1 ops=sharded", {}),
    ("sharded_general_mse", "w=784,64,10 max_rows=128 loss=1 world=2 rank=1 loss_out=0 ops=sharded", {}),
    ("sharded_general_mnist_momentum", "w=%s max_rows=128 opt=2 world=2 rank=1 ops=sharded" % MNIST, {}),
    ("sharded_bucketed_adam", "w=%s max_rows=128 world=2 rank=1 p2p=1 ops=sharded" % MNIST, {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bucketed_sgd", "w=%s max_rows=128 opt=0 world=2 rank=1 ops=sharded" % MNIST, {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bucketed_sgd_no_loss_out", "w=784,64,10 max_rows=128 opt=0 world=2 loss_out=0 ops=sharded", {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bucketed_fail_in_backward", "w=%s max_rows=128 world=2 rank=1 fail_at=14 ops=sharded" % MNIST, {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bucketed_fail_in_adam", "w=%s max_rows=128 world=2 rank=1 fail_at=21 ops=sharded" % MNIST, {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bucketed_fail_in_wait", "w=%s max_rows=128 world=2 rank=1 fail_at=20 ops=sharded" % MNIST, {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bf16_unsharded_optimizer", "w=64,63,64 max_rows=64 loss=1 dtype=bf16 world=2 rank=1 ops=sharded", {}),
    ("sharded_bf16_unsharded_bucketed", "w=64,63,64 max_rows=64 loss=1 dtype=bf16 world=2 rank=1 ops=sharded", {"TNN_BUCKET_BYTES": "1"}),
    ("sharded_bf16_zero_w2", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 ops=gather,sharded,masters,sharded,gather,masters,gather" % B16, {}),
    ("sharded_bf16_zero_w1", "w=%s max_rows=64 loss=1 dtype=bf16 world=1 loss_out=0 ops=sharded,masters" % B16, {}),
    ("sharded_bf16_zero_world_changed", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 ops=sharded,world:4,gather,sync,masters" % B16, {}),
    ("sharded_bf16_zero_fail_before_chain", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 fail_at=10 ops=sharded" % B16, {}),
    ("sharded_bf16_zero_fail_in_chain", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 fail_at=16 ops=sharded" % B16, {}),
    ("sharded_bf16_zero_fail_at_second_chain_begin", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 fail_at=23 ops=sharded" % B16, {}),
    ("sharded_bf16_zero_fail_in_second_chain", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 fail_at=24 ops=sharded" % B16, {}),
    ("sharded_bf16_zero_fail_in_wait", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 fail_at=33 ops=sharded" % B16, {}),
    ("sharded_bf16_zero_fail_after_chains", "w=%s max_rows=64 loss=1 dtype=bf16 world=2 rank=1 fail_at=29 ops=sharded" % B16, {}),
    # ---- phase entry points
    ("phases_f32", "w=784,64,10 max_rows=128 ops=forward,forward_stats,backward,update", {}),
    ("phases_f32_mse_rmsprop", "w=784,64,10 max_rows=128 loss=1 opt=3 loss_out=0 ops=forward,forward_stats,backward,update", {}),
    ("phases_bf16", "w=%s max_rows=64 loss=1 dtype=bf16 ops=sync,forward,forward_stats,backward,update,gather" % B16, {}),
    ("phases_bf16_no_loss_out", "w=%s max_rows=64 loss=1 dtype=bf16 loss_out=0 ops=forward,backward" % B16, {}),
]


def run_case(exe, args, env):
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("TNN_")}
    child_env.update(env)
    return subprocess.run([exe] + args.split(), env=child_env, check=True, capture_output=True, text=True).stdout


def trace_all(exe):
    out = []
    for name, args, env in CASES:
        head = "== %s: %s" % (name, args)
        if env:
            head += " | " + " ".join("%s=%s" % kv for kv in sorted(env.items()))
        out.append(head + "\n" + run_case(exe, args, env))
    return out


def sections(text):
    return ["== " + s for s in text.split("== ")[1:]]


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    return trace_all(build_harness(tmp_path_factory.mktemp("mlp_trace")))


def test_launch_sequences_match_the_recorded_ones(traces):
    want = sections(open(FIXTURE).read())
    assert [s.split(":")[0] for s in want] == [s.split(":")[0] for s in traces], "case list and fixture differ"
    for got, exp in zip(traces, want):
        if got != exp:
            diff = "\n".join(difflib.unified_diff(exp.splitlines(), got.splitlines(), "recorded", "now", lineterm=""))
            pytest.fail("launch sequence changed\n%s\n---- full new trace\n%s" % (diff, got))


def test_launch_counts_of_the_headline_forms(traces):
    by_name = {s.split(":")[0][3:]: s for s in traces}
    def calls(name):
        return [int(n) for n in re.findall(r"calls_in_last_step=(\d+)", by_name[name])]
    assert calls("step_mnist_128") == [4, 4] and calls("step_mnist_32") == [4]          # 2L - 2
    assert calls("step_deep_generic_head") == [8]
    assert calls("step_rowblocks_256_tuned") == [4] and calls("step_rowblocks_300_generic") == [8]
    assert calls("step_mnist_window_1_2") == [4, 4]                  # skipped calls are counted too


def test_every_case_ran_to_its_end(traces):
    for s in traces:
        assert "unknown op" not in s and (s.count("\n-- ") == s.count("\nrc=") + s.count("\n-- world:")), s


if __name__ == "__main__":
    import argparse
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", default=SOURCE)
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--cxxflags", default="", help="extra compiler flags, e.g. -fsanitize=address,undefined")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        text = "".join(trace_all(build_harness(d, a.source, a.cxxflags.split())))
    if a.record:
        open(FIXTURE, "w").write(text)
    else:
        sys.stdout.write(text)

"""xGMI peer-to-peer transport (csrc/tnn_p2p.hip) on the GPU box: a one-rank group in-process (kernels, hipGraph
replay, routing under tnn_allreduce / tnn_allgather) and a real two-process group sharing the box's single GPU
(IPC mapping, flag barriers, sharded training against the reference's bs=1024 fixture) — see tests/p2p_worker.py."""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import tinynn_autograd_amd as tn
from conftest import ROOT


@pytest.mark.gpu
def test_p2p_world1_collectives_and_graph():
    from tinynn_autograd_amd.dist import XgmiCommunicator
    from tinynn_autograd_amd import _lib
    comm = XgmiCommunicator(0, 1, p2p_bytes=1 << 20)
    try:
        assert comm.p2p_status() == {"connected": True, "enabled": True, "dead": False}
        assert comm.p2p_selftest(sizes=(1, 3, 1000, 235147), rounds=2)
        rs = np.random.RandomState(5)
        for n in (1, 2, 7, 64, 4099, 262144):                    # ragged tails, up to the mapped capacity
            x = rs.randn(n).astype(np.float32)
            d = tn.asarray(x)
            comm.allreduce(d)
            assert np.array_equal(np.asarray(d), x), n
        big = tn.asarray(np.ones(300000, np.float32))              # over capacity and no RCCL communicator: loud
        with pytest.raises(RuntimeError):
            comm.allreduce(big)
        g = comm.allgather(tn.asarray(np.array([1.5, -2.5], np.float32)))
        assert np.array_equal(np.asarray(g), [[1.5, -2.5]])
        d = tn.asarray(np.arange(1000, dtype=np.float32))
        graph = _lib.Graph()
        with graph:
            for _ in range(4):
                comm.allreduce(d)
                d *= 2.0
        for _ in range(3):
            graph.launch()
        assert np.array_equal(np.asarray(d), np.arange(1000, dtype=np.float32) * 2.0 ** 12)
        assert not comm.p2p_status()["dead"]
    finally:
        comm.close()


@pytest.mark.gpu
def test_sharded_trainer_on_p2p_world1_matches_reference_fixture():
    """The 8-launch data-parallel step (exchange inside the loss kernel, Adam inside the all-reduce kernel) on a
    one-rank group: every collective is the identity, so the reference's single-process trajectory must come out —
    eagerly and replayed from a hipGraph."""
    import helpers as H
    from tinynn_autograd_amd.dist import XgmiCommunicator
    comm = XgmiCommunicator(0, 1, p2p_bytes=2 << 20)
    try:
        cfg, gold = H.load_traj("A_adam")
        w = cfg["widths"]
        model, _ = H.build_model(cfg)
        trainer = tn.trainer_from_net(model.net, max_rows=cfg["m"], lr=cfg["lr"], comm=comm, force_dp=True)
        data = list(H.batches(cfg["data_seed"], 8, cfg["m"], w[0], w[-1], cfg["loss"]))
        for s in range(4):
            x, y = data[s]
            np.testing.assert_allclose(float(trainer.step(tn.asarray(x), tn.asarray(y))), gold["loss"][s], rtol=1e-5)
        graph = trainer.capture_steps([(tn.asarray(x), tn.asarray(y)) for x, y in data[4:8]])
        np.testing.assert_allclose(np.asarray(graph.launch()), gold["loss"][4:8], rtol=1e-5)
        assert not comm.p2p_status()["dead"]
    finally:
        comm.close()


@pytest.mark.gpu
def test_sharded_trainer_on_p2p_world1_equals_the_single_gpu_trainer():
    """The 4-launch data-parallel step — the first layer's backward pushes its tiles straight into the all-reduce's receive
    slots and carries stages B / C and Adam (tnn_dense_bwd_first_allreduce_adam) — on a one-rank group against the
    single-GPU trainer on the same batches: full, ragged and odd row counts; a four-layer net; 320 rows (the two launches
    the fused one replaces); a single row; eager, then replayed from a hipGraph."""
    from tinynn_autograd_amd.dist import XgmiCommunicator
    from tinynn_autograd_amd.fused import MLPTrainer
    comm = XgmiCommunicator(0, 1, p2p_bytes=2 << 20)
    try:
        for widths, rows in (([784, 256, 128, 10], 128), ([784, 256, 128, 10], 80), ([784, 256, 128, 10], 37),
                             ([60, 48, 64, 128, 10], 128), ([784, 256, 128, 10], 320), ([40, 16, 128, 10], 1),
                             ([784, 256, 128, 10], 1024), ([784, 256, 128, 10], 520)):        # (32 x 32 tile form of the fused launch)
            rs = np.random.RandomState(rows + len(widths))
            batches = [(tn.asarray(rs.uniform(-1, 1, (rows, widths[0])).astype(np.float32)),
                        tn.asarray(np.eye(widths[-1], dtype=np.float32)[rs.randint(0, widths[-1], rows)])) for _ in range(6)]
            layers = [{"w": rs.uniform(-0.1, 0.1, (a, b)).astype(np.float32), "b": rs.uniform(-0.1, 0.1, (1, b)).astype(np.float32)}
                      for a, b in zip(widths[:-1], widths[1:])]
            solo = MLPTrainer(widths, rows, loss="softmax_nll", optimizer="adam", lr=1e-3)
            dp = MLPTrainer(widths, rows, loss="softmax_nll", optimizer="adam", lr=1e-3, comm=comm, force_dp=True)
            solo.set_parameters(layers)
            dp.set_parameters(layers)
            assert np.array_equal(np.asarray(solo.flat_parameters()), np.asarray(dp.flat_parameters()))
            for x, y in batches[:3]:
                np.testing.assert_allclose(float(dp.step(x, y)), float(solo.step(x, y)), rtol=1e-5, err_msg=str((widths, rows)))
            graph = dp.capture_steps(batches[3:])
            losses = np.asarray(graph.launch())
            for i, (x, y) in enumerate(batches[3:]):
                np.testing.assert_allclose(losses[i], float(solo.step(x, y)), rtol=1e-5, err_msg=str((widths, rows, i)))
            # parameters: Adam divides by sqrt(v) — where a gradient is all rounding noise (|g| ~ 1e-9) the two step forms'
            # different summation orders move an update by a visible fraction of lr; 6 steps of lr = 1e-3 bound that at 6e-3,
            # observed 1.1e-5 on 11 of 235 146 elements
            np.testing.assert_allclose(np.asarray(dp.flat_parameters()), np.asarray(solo.flat_parameters()), rtol=1e-5, atol=5e-5,
                                       err_msg=str((widths, rows)))
        assert not comm.p2p_status()["dead"]
    finally:
        comm.close()


@pytest.mark.gpu
def test_p2p_eight_processes_the_n8_point():
    """configs[3] as the driver's N = 8 run shards it — global batch 1024, 128 rows per rank — with EIGHT ranks on the box's
    one GPU: the 5-launch sharded step (statistics reduced and exchanged by the last workgroup of the forward launch, tagged
    all-reduce with the Adam tail) reproduces the reference's bs-1024 trajectory, replicas identical, timeout drill green.
    Only one workgroup per rank ever waits for a peer outside the all-reduce, so the ranks cannot starve each other."""
    # (8 x 272 workgroups of the head launch do not fit the GPU together: on a SHARED device the step keeps the exchange at the tail of
    # the forward launch, where one workgroup per rank waits; with one process per GPU it takes the deferred form)
    _run_p2p_workers(8, "D_adam", TNN_P2P_TEST_EXPECT_XCHG="0")


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_optimizer_step_with_ranks_sharing_the_gpu(world):
    """configs[4]'s multi-rank leg ON THE HIP LIBRARY with rank > 0: the bf16 trainer's sharded-optimizer step (mlp16_step_zero —
    reduce-scatter of the bf16 dW, Adam on the owned rows, all-gather of the bf16 rows) at 1024-wide x 2 layers with 2 and 4 ranks on
    the box's one GPU, collectives on the peer-to-peer transport's bulk path (RCCL refuses ranks that share a device).  The GPU
    twin of tests/dp_hook_worker.py mode "E": see tests/p2p_zero_worker.py."""
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), TNN_DEVICE="0", WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TNN_P2P_TIMEOUT_MS="20000",
                   HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "p2p_zero_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=400)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (rank, out[-3000:])
        assert "p2p_zero_worker rank %d/%d ok" % (rank, world) in out


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_p2p_workers(world, traj="D_adam", **extra_env):
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), TNN_DEVICE="0", WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), TNN_P2P_TIMEOUT_MS="3000",
                   TNN_P2P_TEST_TIMEOUT="1", TNN_P2P_TEST_TRAJ=traj,
                   HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONDONTWRITEBYTECODE="1")
        env.update(extra_env)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "p2p_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (rank, out[-3000:])
        assert "p2p_worker rank %d/%d ok" % (rank, world) in out


@pytest.mark.gpu
def test_p2p_two_processes_share_the_gpu():
    """512 rows per rank: the 8-launch sharded step (exchange inside the one-workgroup loss kernel)."""
    _run_p2p_workers(2)


@pytest.mark.gpu
def test_p2p_two_processes_five_launch_step():
    """The reference's bs-128 trajectory split over two ranks (64 rows each): the 5-launch sharded step — the last
    workgroup of the hidden layer's forward reduces the shard's softmax statistics and exchanges them with the peer
    (tnn_dense_fwd_head_partials_stats), the head launch only reads the merged pair — eager, replayed from a hipGraph,
    replicas identical, and the timeout drill.  One workgroup per rank waits for a peer, so ranks sharing a GPU cannot
    starve each other (`TNN_P2P_TEST_TRAJ=D_adam` with 8 workers runs the N = 8 shape on one GPU the same way)."""
    _run_p2p_workers(2, "A_adam", TNN_P2P_TEST_EXPECT_XCHG="1")      # 2 x 208 workgroups fit the GPU: the DEFERRED exchange


@pytest.mark.gpu
def test_p2p_statistics_exchange_at_the_tail_of_the_forward_launch_still_works():
    """The data-parallel step takes the DEFERRED statistics exchange by default (round 6: the head launch pushes the shard's
    {max, sum-exp} pair and merges the ranks' pairs itself, tnn_mlp_head_bwd_tick_xchg).  TNN_DP_XCHG=0 selects the round-5
    form — reduced, exchanged and merged by the last workgroup of the forward launch — which stays the form of generic heads
    above 128 rows per rank: both must reproduce the reference's trajectories (128 rows per rank at 8 ranks, 512 at 2)."""
    _run_p2p_workers(2, "A_adam", TNN_DP_XCHG="0")
    _run_p2p_workers(2, "D_adam", TNN_DP_XCHG="0")


@pytest.mark.gpu
def test_p2p_four_processes_quarter_batches():
    """configs[3] split over FOUR ranks sharing the box's GPU (256 rows per rank: the row-panel forward leaves 16 panel pairs,
    the row-blocked head launch merges them, pushes the shard's pair and merges the four ranks' pairs) and the bs-128
    trajectory split four ways (32 rows per rank)."""
    _run_p2p_workers(4, "D_adam")
    _run_p2p_workers(4, "A_adam")


@pytest.mark.gpu
def test_p2p_reference_example_net_two_and_eight_ranks():
    """The reference's OWN example net (examples/mnist/run.py:59-69, tests/golden/traj_R_example_D.npz: bs 1024) split over
    2 ranks (512 rows each: the generic merged head walks four blocks of 128) and 8 ranks (128 rows each) sharing the box's
    one GPU — the merged 2L - 2 launch data-parallel step for a head that is NOT the benchmark's 128 -> 10, eager and captured,
    replicas identical, timeout drill."""
    _run_p2p_workers(2, "R_example_D")                                   # 512 rows per rank: a generic head above 128 rows keeps the forward tail
    _run_p2p_workers(8, "R_example_D", TNN_P2P_TEST_EXPECT_XCHG="1")     # 128 rows per rank, 8 x 52 workgroups: the DEFERRED exchange, generic kernel


@pytest.mark.gpu
def test_bench_two_ranks_under_torchrun_share_the_gpu():
    """bench.py's N > 1 flow exactly as the driver launches it (python -m torch.distributed.run ... bench.py --gpus 2),
    with both ranks on the box's one GPU and the peer-to-peer-only communicator (RCCL refuses ranks that share a
    device): rendezvous, transport self-test vote, sharded steps in hipGraphs, max-over-ranks timing, the replicas
    check, and exactly ONE JSON line on stdout from rank 0."""
    import json
    env = dict(os.environ, TNN_COMM="xgmi", TNN_DEVICE="0", TNN_P2P_TIMEOUT_MS="20000", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "128",
           "--warmup", "64", "--full"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 128 and d["warmup"] == 64 and d["scaling"] == "weak"
    # `value` is on the N = 1 line's definition: 128 rows per rank (N = 8 is then configs[3]'s global batch 1024)
    assert d["config"]["global_batch"] == 256 and d["config"]["rows_per_rank"] == 128 and d["config"]["parallelism"] == "dp2"
    assert d["exit_code"] == 0 and d["timing"]["segments_per_repeat"] >= 1
    coll = d["config"]["collectives"]
    assert coll["used"] == "xgmi-p2p" and "rccl" not in coll            # TNN_COMM=xgmi: no RCCL communicator exists
    p2p = coll["xgmi_p2p"]
    assert p2p["replicas_identical"] and p2p["verified_after_run"] and not p2p["barrier_timed_out"] and p2p["graph_captured"]
    assert d["value"] == p2p["value"] > 0
    # the sharded step on this transport reproduces the REFERENCE's bs-1024 losses (traj_D_adam, all 5 steps; no reference
    # fixture exists at global batch 256, so the check runs at config D's split: 512 rows per rank)
    chk = d["parity_vs_reference_fixture"]
    assert chk["ok"] and chk["steps"] == 5 and "traj_D_adam" in chk["fixture"] and chk["max_rel_err"] <= 1e-5
    assert chk["global_batch"] == 1024 and chk["rows_per_rank"] == 512
    # both curves on the one line: this N's weak point (= value), the strong point, the single-GPU references of both
    assert d["weak_scaling"]["global_batch"] == 256 and d["weak_scaling"]["value"] == d["value"]
    assert d["strong_scaling"]["global_batch"] == 1024 and d["strong_scaling"]["rows_per_rank"] == 512
    # the third curve (1024 rows per rank) with its own single-GPU reference and speedup
    w3 = d["weak_scaling_1024"]
    assert w3["global_batch"] == 2048 and w3["rows_per_rank"] == 1024 and w3["replicas_identical"] and w3["speedup_vs_n1"] > 0
    assert abs(w3["speedup_vs_n1"] - w3["value"] / d["single_gpu_bs1024"]["value"]) < 1e-3
    # the step form that was TIMED (128 rows per rank) is checked too, against the single-GPU trainer on the whole batch
    pt = d["parity_at_timed_rows"]
    assert pt["ok"] and pt["rows_per_rank"] == 128 and pt["global_batch"] == 256 and pt["replicas_identical"] and pt["max_rel_err"] <= 1e-5
    assert "512" not in chk["step_form"] and "4 block" in chk["step_form"] and "1 block" in pt["step_form"]
    # what the run stood on: RCCL version, peer access, self-tests before and after, per-collective latencies, which transport and why
    mg = d["multi_gpu"]
    assert mg["world"] == 2 and mg["value_from"] == "xgmi-p2p" and mg["why"] and mg["ranks_share_a_device"]
    assert mg["selftest_before_timed_runs"] == {"xgmi_p2p": True} and mg["selftest_after_timed_runs"] == {"xgmi_p2p": True}
    lat = mg["collective_latency"]["xgmi_p2p"]
    assert lat["allreduce_940588_B"] > 0 and lat["allgather_2_floats_per_rank"] > 0
    assert "can_access_peer" in mg["topology"] and isinstance(mg["rccl_version"], str)
    assert d["strong_scaling"]["replicas_identical"] and d["single_gpu_bs1024"]["value"] > 0 and d["single_gpu_bs128"]["value"] > 0
    assert abs(d["value"] / d["single_gpu_bs128"]["value"] - d["speedup_vs_n1"]) <= 1e-3 * d["speedup_vs_n1"]


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [2, 4])
def test_bench_gpus_2_launches_its_own_ranks(gpus):
    """`python3 bench.py --gpus N ...` with NO launcher (the form the driver uses for N = 1): the parent, which never
    touches the GPU, starts the ranks itself, relays rank 0's one JSON line and passes the children's status on.  `value` is on
    ONE definition at every N — weak scaling, 128 rows per rank, global batch 128 N — and `speedup_vs_n1` is that value over
    the 128-row single-GPU step measured on rank 0 of the same run.  The strong curve (configs[3]'s global batch 1024 split
    over the ranks: 512 / 256 rows per rank at N = 2 / 4 — the data-parallel 5-launch step whose merged head launch walks the
    rows in blocks of 128) rides beside it with its own speedup."""
    import json
    env = dict(os.environ, TNN_COMM="xgmi", TNN_DEVICE="0", TNN_P2P_TIMEOUT_MS="20000", HSA_ENABLE_IPC_MODE_LEGACY="0",
               PYTHONDONTWRITEBYTECODE="1")
    if gpus > 2:
        env["TNN_BENCH_CONFIG_E"] = "0"                 # four 8192-wide bf16 trainers on one GPU: covered at N = 2
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20", "--warmup", "5", "--full"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == gpus and d["steps"] == 20 and d["warmup"] == 5 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 128 * gpus and d["config"]["rows_per_rank"] == 128
    assert d["parity_vs_reference_fixture"]["ok"] and d["exit_code"] == 0
    assert d["config"]["collectives"]["xgmi_p2p"]["replicas_identical"]
    # the line's own N = 1 reference and the speedup computed from it, on the line's own definition
    n1 = d["single_gpu_bs128"]["value"]
    assert abs(d["value"] / n1 - d["speedup_vs_n1"]) <= 1e-3 * d["speedup_vs_n1"]
    assert d["weak_scaling"]["rows_per_rank"] == 128 and d["weak_scaling"]["global_batch"] == 128 * gpus
    assert abs(d["weak_scaling"]["speedup_vs_n1"] - d["speedup_vs_n1"]) < 1e-9
    st = d["strong_scaling"]
    assert st["global_batch"] == 1024 and st["rows_per_rank"] == 1024 // gpus and "note" in st
    assert abs(st["value"] / d["single_gpu_bs1024"]["value"] - st["speedup_vs_n1"]) <= 1e-3 * st["speedup_vs_n1"]


@pytest.mark.gpu
def test_bench_self_launch_fails_fast_when_a_rank_dies():
    """One of the self-launched ranks exits right after the rendezvous: the launcher ends the other rank (by PID) and
    returns a non-zero status well inside the timeout instead of hanging in a collective."""
    import time
    env = dict(os.environ, TNN_COMM="xgmi", TNN_DEVICE="0", TNN_P2P_TIMEOUT_MS="5000", HSA_ENABLE_IPC_MODE_LEGACY="0",
               TNN_BENCH_TEST_EXIT_RANK="1", PYTHONDONTWRITEBYTECODE="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode != 0
    assert time.time() - t0 < 240
    assert "rank 1 exited with code 9" in r.stderr


@pytest.mark.gpu
def test_bench_single_gpu_line_has_the_contract_objects(tmp_path):
    """The driver's N = 1 command with --full: one JSON line with the median-of-repeats protocol, the latency-bound roofline
    with the per-launch event times, the 4096 GEMM roofline, config C's whole step, the drop-in API paths, the strong-scaling
    N = 1 point (= `--workload A --rows 1024`), the parity check against the reference fixture and both CPU legs.  Its
    --dump-outputs are those of a plain run with the same arguments."""
    import json
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full",
                        "--dump-outputs", str(tmp_path / "full")],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["config"]["global_batch"] == 128
    assert "configs[1]" in d["config"]["workload"] and d["exit_code"] == 0
    t = d["timing"]
    assert t["min_ms_per_step"] <= d["ms_per_step"] <= t["max_ms_per_step"] and t["timed_ms_per_repeat"] >= 45.0
    roof = d["roofline"]
    assert roof["bound"] == "latency" and roof["launches_per_step"] == len(roof["per_launch_us"]) and 0 < roof["frac"] <= 1
    assert roof["gemm_frac"] > 0 and d["roofline_gemm4096"]["bound"] == "mfma" and d["roofline_gemm4096"]["frac"] > 0.5
    assert d["parity_vs_reference_fixture"]["ok"] and "traj_A_adam" in d["parity_vs_reference_fixture"]["fixture"]
    assert d["paths"]["ops_eager"]["value"] > 0 and d["paths"]["ops_graph"]["value"] > d["paths"]["ops_eager"]["value"]
    assert d["config_C"]["value"] > 0 and d["strong_scaling"]["global_batch"] == 1024
    ex = d["reference_example_net"]                       # examples/mnist/run.py:59-69, the trainer's generic step form
    assert ex["widths"] == "784-200-100-70-30-10" and ex["value"] > 0 and ex["launches_per_step"] == 8     # 2 L - 2
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["single_thread"]["cores"] == 1 and cpu["cpu_model"]
    # `value` is the host's best leg (all BLAS threads / 8 / 1), every leg stays on the line with its thread count
    assert cpu["value"] >= cpu["single_thread"]["value"] and cpu["value"] >= cpu["all_threads"]["value"]
    assert cpu["cores"] == cpu[cpu["best_leg"]]["cores"]
    # `--workload A --rows 1024` is the same measurement as the strong-scaling N = 1 point
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                         "--rows", "1024", "--no-extras", "--full"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-3000:]
    d2 = json.loads([l for l in r2.stdout.splitlines() if l.strip()][0])
    assert d2["config"]["global_batch"] == 1024
    assert abs(d2["value"] / d["strong_scaling"]["value"] - 1.0) < 0.1
    # the same arguments without --full: the same outputs (--full times its repeats only after the plain run's steps)
    r3 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                         "--dump-outputs", str(tmp_path / "plain")], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=600)
    assert r3.returncode == 0, r3.stderr[-3000:]
    names = sorted(p.name for p in (tmp_path / "full").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "plain").iterdir()) and "loss.npy" in names and "w0.npy" in names
    for n in names:
        np.testing.assert_array_equal(np.load(str(tmp_path / "full" / n)), np.load(str(tmp_path / "plain" / n)), err_msg=n)


@pytest.mark.gpu
def test_bench_plain_run_times_exactly_the_given_steps_and_dumps_its_outputs(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W` without --full: the headline alone, N steps in one timed region after W
    warm-up steps, and --dump-outputs writes what that path computed in its last step — the loss and every layer's weight and
    bias after W + N steps, as an eager trainer on the same seeded batches computes them."""
    import json
    from bench.common import WIDTHS_A
    from bench.runners import FusedRun
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    warmup, steps = 7, 150                               # neither a multiple of the 64-step chunk: head and tail segments
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["exit_code"] == 0 and d["value"] > 0
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    t = d["timing"]
    assert t["segments_per_repeat"] == 1 and "one timed region of %d steps" % steps in t["statistic"]
    assert abs(t["timed_ms_per_repeat"] - steps * d["ms_per_step"]) <= 0.01
    assert abs(d["value"] - 128 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for key in ("roofline", "cpu_baseline", "parity_vs_reference_fixture", "config_C", "epoch_loop", "box", "strong_scaling"):
        assert key not in d, key
    ref = FusedRun(WIDTHS_A, 128, "softmax_nll", 64, use_graph=False)
    ref.last_loss = [ref.eager_step(i) for i in range(warmup + steps)][-1]
    want = dict(ref.outputs())
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(n + ".npy" for n in want)
    assert sum(p.stat().st_size for p in tmp_path.iterdir()) <= 64 << 20
    np.testing.assert_allclose(np.load(str(tmp_path / "loss.npy")), [d["final_loss"]], rtol=1e-5)
    for n, a in want.items():
        got = np.load(str(tmp_path / (n + ".npy")))
        assert got.dtype == np.float32 and got.shape == a.shape, n
        np.testing.assert_allclose(got, a, rtol=1e-5, atol=1e-6, err_msg=n)

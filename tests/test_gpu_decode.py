"""csrc/tnn_decode.hip on the MI355X: decode attention (native against the float64 oracle under its derived bounds and against
the composed route under the sum of both bounds, the appended row bit for bit, nothing else written, NaN beyond the live
prefix never read, identical bits on a repeated call) and token sampling (tokens EQUAL the oracle's for u with the margin),
then generation end to end against the fixture.  Shapes are the smallest at which a path can go wrong: lengths around the
chunk of 64 keys, every split count of a 5-chunk prefix, head dimensions on both sides of the 16-byte pack and of the 64
columns one lane group covers with element accesses."""

import numpy as np
import pytest

import attn_oracle as ao
import decode_oracle as do
import decode_support as ds
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import decoding as dc, device_array as da, generation as gen

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
TMAX = 200


@pytest.fixture(scope="module")
def golden():
    return ds.load_golden()


def check_decode(case, dtype, splits, unaligned=False, what=""):
    """Native under the oracle's bound, composed under the plain bound, the two within the sum; the caches bit for bit."""
    tn.set_default_float(dtype)
    plan = dc.plan_decode(case["q"].shape, case["k_cache"].shape, case["v_cache"].shape, case["length"],
                          case["k_new"] is not None, layout=case["layout"], splits=splits)
    res = ds.reference(case, dtype, plan.splits)
    o, kc, vc = ds.run_decode("native", case, dtype, splits, unaligned)
    assert o.dtype == dtype and np.isfinite(o).all(), what
    ao.assert_within(o, res.values["o"], res.bounds["o"], "%s native" % what)
    want_k, want_v = ds.expected_caches(case, dtype)
    assert np.array_equal(ds.bits(kc), ds.bits(want_k)) and np.array_equal(ds.bits(vc), ds.bits(want_v)), what
    o2, kc2, vc2 = ds.run_decode("native", case, dtype, splits, unaligned)
    assert np.array_equal(ds.bits(o), ds.bits(o2)), "%s: a repeated call gives other bits" % what
    oc, kcc, vcc = ds.run_decode("composed", case, dtype, None, unaligned)
    ao.assert_within(oc, res.values["o"], res.bounds["o"], "%s composed" % what)
    assert np.array_equal(ds.bits(kcc), ds.bits(want_k)) and np.array_equal(ds.bits(vcc), ds.bits(want_v)), what
    assert (np.abs(o.astype(np.float64) - oc) <= 2 * res.bounds["o"]).all(), "%s native against composed" % what
    return plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 129, TMAX - 1])
def test_lengths_around_the_chunk(length, dtype):
    """The planner's own split (B H = 3: every chunk its own workgroup), both layouts."""
    for layout in dc.LAYOUTS:
        case = ds.make_case(do.case_seed("len%d%s" % (length, layout)), layout, 3, 1, TMAX, length, 16, 24, True, dtype)
        plan = check_decode(case, dtype, None, what="len %d %s" % (length, layout))
        assert plan.splits == plan.chunks == length // 64 + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splits", [1, 2, 3, 5])
def test_every_split_of_five_chunks(splits, dtype):
    """300 + 1 keys are 5 chunks: 2 and 3 splits get runs of unequal length, 5 is the maximum, 6 is refused."""
    case = ds.make_case(do.case_seed("splits"), "bthd", 1, 3, 320, 300, 64, 32, True, dtype)
    plan = check_decode(case, dtype, splits, what="splits %d" % splits)
    assert plan.chunks == 5 and sorted(set(b - a for a, b in plan.runs())) == {1: [5], 2: [2, 3], 3: [1, 2], 5: [1]}[splits]
    with pytest.raises(ValueError, match="splits 6 outside"):
        ds.run_decode("native", case, dtype, 6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_chunks_than_splits_allowed(dtype):
    """301 chunks for one (b, h): the planner clamps at MAX_SPLITS = 256 workgroups, whose runs are one or two chunks long,
    and the combine walks 256 workspace records."""
    case = ds.make_case(do.case_seed("clamp"), "bhtd", 1, 1, 64 * 301, 64 * 300 + 5, 4, 8, True, dtype)
    plan = check_decode(case, dtype, None, what="301 chunks")
    assert plan.chunks == 301 and plan.splits == dc.MAX_SPLITS and sorted(set(b - a for a, b in plan.runs())) == [1, 2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_the_fwd_route(layout, dtype):
    """route="fwd" — a sliced append plus tnn_attn_fwd with Tq = 1 striding into the cache, where the planner's rules send a
    region that the probe found slower — gives the same result under the plain bound and the same caches."""
    tn.set_default_float(dtype)
    for length, append in ((70, True), (96, False)):
        case = ds.make_case(do.case_seed("fwd%d%s" % (length, layout)), layout, 2, 3, 96, length, 16, 24, append, dtype)
        res = ds.reference(case, dtype, 1)
        o, kc, vc = ds.run_decode("fwd", case, dtype)
        assert np.isfinite(o).all()
        ao.assert_within(o, res.values["o"], res.bounds["o"], "fwd %s %d" % (layout, length))
        want_k, want_v = ds.expected_caches(case, dtype)
        assert np.array_equal(ds.bits(kc), ds.bits(want_k)) and np.array_equal(ds.bits(vc), ds.bits(want_v))


def test_the_library_refuses_what_the_planner_refuses():
    """The raw entry point, past the planner: too many splits, a full cache, a missing v_new."""
    from tinynn_autograd_amd import _lib
    lib = _lib.get()
    q, k, v, o = (tn.zeros(s, np.float32) for s in ((1, 1, 4), (1, 8, 1, 4), (1, 8, 1, 4), (1, 1, 4)))
    strides = da._i64arr((4, 4, 0) * 3 + (32, 4, 4) * 2 + (4, 4, 0))
    for args, msg in ((dict(length=7, splits=2), "splits 2 outside"), (dict(length=8, splits=1), "len 8 with a cache of 8"),
                      (dict(length=3, splits=1, v_new=None), "come together")):
        with pytest.raises(_lib.TnnError, match=msg):
            lib.decode_attn(q._ptr, q._ptr, q._ptr if "v_new" not in args else None, k._ptr, v._ptr, o._ptr, None, 0, 1, 1,
                            args["length"], 8, 4, 4, strides, 0.5, args["splits"], 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dv,b,h", [(1, 2, 1, 1), (3, 5, 3, 1), (4, 8, 1, 3), (5, 3, 1, 1), (16, 4, 3, 1), (17, 16, 1, 3),
                                      (64, 128, 1, 1), (65, 64, 1, 3), (128, 65, 3, 1)])
def test_head_dimensions(d, dv, b, h, dtype):
    """Wide accesses (4 / 8, 16 / 4, 64 / 128), element accesses with one pack per lane and, beyond 64 columns, two; 70 + 1
    keys in two splits, both layouts."""
    for layout in dc.LAYOUTS:
        case = ds.make_case(do.case_seed("dims%d.%d%s" % (d, dv, layout)), layout, b, h, 96, 70, d, dv, True, dtype)
        check_decode(case, dtype, 2, what="D %d Dv %d %s" % (d, dv, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_element_aligned_bases_and_no_append(layout, dtype):
    """Bases that are only element-aligned take the element accesses; without k_new / v_new the keys are [0, length) and the
    caches are not written (length == Tmax is then legal)."""
    case = ds.make_case(do.case_seed("unaligned" + layout), layout, 1, 3, 96, 70, 16, 8, True, dtype)
    check_decode(case, dtype, 2, unaligned=True, what="unaligned %s" % layout)
    for length in (1, 64, 96):
        case = ds.make_case(do.case_seed("null%d%s" % (length, layout)), layout, 3, 1, 96, length, 16, 8, False, dtype)
        check_decode(case, dtype, None, what="no append, length %d %s" % (length, layout))
        check_decode(case, dtype, None, unaligned=True, what="no append, unaligned, length %d %s" % (length, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(do.DECODE_CASES))
def test_the_fixtures_cases(golden, name, dtype):
    case = do.decode_case(name, np.float32)                    # (the fixture's inputs are float32 values in either run)
    splits = case.pop("splits")
    check_decode(case, dtype, splits, what=name)
    res = ds.reference(case, dtype, splits)
    np.testing.assert_allclose(res.values["o"], golden["decode." + name], rtol=1e-12, atol=1e-300)


# ---------------------------------------------------------------------- sampling
def sample_rows_of(rs, m, v, kind, dtype):
    if kind == "normal":
        return do.sample_inputs(rs, m, v, 3.0, dtype)
    if kind == "ties":                                         # few distinct values: duplicates straddle every threshold
        return rs.randint(0, 4, (m, v)).astype(dtype)
    if kind == "constant":
        return np.full((m, v), 1.5, dtype=dtype)
    x = do.sample_inputs(rs, m, v, 3.0, dtype)                 # "inf": -inf entries, the first and the last column among them
    x[:, rs.rand(v) < 0.3] = -np.inf
    if v > 2:
        x[:, 0] = x[:, -1] = -np.inf
    x[:, v // 2] = 1.0
    return x


def check_sample(x, temperature, top_k, dtype, rs, what, u=None):
    res = do.sample_reference(x, temperature, top_k, dtype)
    if temperature == 0.0:
        want = res.argmax
    else:
        u = do.draw_u(res, rs, dtype) if u is None else np.full(x.shape[0], u, dtype=dtype)
        want = res.tokens(u)
        assert (res.margins(u, want) > do.MARGIN).all(), "%s: u without the margin (a condition on the inputs)" % what
    got = ds.run_sample("native", x, u, temperature, top_k, dtype)
    assert np.array_equal(got, want), "%s: native %s, oracle %s" % (what, got, want)
    assert np.array_equal(ds.run_sample("composed", x, u, temperature, top_k, dtype), want), "%s composed" % what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("v", [1, 2, 63, 64, 65, 1023, 1025, 4097])
def test_sampling_equals_the_oracle(v, dtype):
    tn.set_default_float(dtype)
    rs = np.random.RandomState(do.case_seed("sample%d" % v))
    top_ks = [None] + sorted({k for k in (1, 2, v - 1, v, v + 1) if k >= 1})
    for i, (top_k, temperature) in enumerate((k, t) for k in top_ks for t in (0.0, 0.5, 1.0, 2.0)):
        m = (1, 3, 5)[i % 3]
        # rows of (nearly) equal weights give every token 1 / n of the unit interval: below 4 cdf_bounds (~ 8 n u each) once n
        # is in the hundreds, so no u has the margin there — those rows go with few kept columns or the greedy rule
        flat_ok = temperature == 0.0 or v <= 65 or (top_k is not None and top_k <= 2)
        for kind in ("normal", "ties", "constant", "inf") if flat_ok else ("normal", "inf"):
            x = sample_rows_of(rs, m, v, kind, dtype)
            check_sample(x, temperature, top_k, dtype, rs, "V %d top_k %s T %g M %d %s" % (v, top_k, temperature, m, kind))


def plateau_rows(rs, m, v, whole, dtype):
    """8 peaks of 8 .. 10 and a PLATEAU of equal values 0 — on every other column (the rest at -30) or, `whole`, on the whole
    background: the peaks own wide intervals, so u has its margin there, while where the peaks lie on the unit interval
    depends on WHICH ties are kept."""
    x = np.full((m, v), 0.0 if whole else -30.0, dtype=dtype)
    if not whole:
        x[:, ::2] = 0.0
    for r in range(m):
        x[r, rs.choice(v, 8, replace=False)] = rs.uniform(8.0, 10.0, 8)
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("v", [1023, 1025, 4097])
def test_sampling_with_many_ties_at_the_threshold(v, dtype):
    """The radix select ends on a value that hundreds of columns share and `need` of them, the lowest indices, are kept
    across several steps of the scan: top_k in the middle of the plateau, and top_k = V - 1 (one tie, the last, dropped)."""
    tn.set_default_float(dtype)
    rs = np.random.RandomState(do.case_seed("plateau%d" % v))
    for whole, top_k in ((False, 8 + (v + 1) // 4), (True, v - 1), (True, 8 + v // 3)):
        for temperature in (1.0, 2.0):
            x = plateau_rows(rs, 3, v, whole, dtype)
            res = do.sample_reference(x, temperature, top_k, dtype)
            ties = [int((res.kept[r] & (x[r] == 0)).sum()) for r in range(3)]
            assert min(ties) == top_k - 8 > 200 and all(res.kept[r][x[r] > 0].all() for r in range(3))
            for _ in range(4):
                check_sample(x, temperature, top_k, dtype, rs, "V %d plateau whole=%s top_k %d T %g" % (v, whole, top_k, temperature))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sampling_at_the_ends_of_the_unit_interval(dtype):
    """u = 0 gives the first kept column of positive weight, u = nextafter(1, 0) the last — through the running sum or the
    rule's fallback; both ends are exact (decode_oracle)."""
    tn.set_default_float(dtype)
    rs = np.random.RandomState(do.case_seed("ends"))
    one = np.nextafter(np.dtype(dtype).type(1), np.dtype(dtype).type(0))
    for v, top_k in ((65, None), (65, 2), (1025, 3), (2, None), (1, None)):
        for holes in (False, True):
            for temperature in (0.5, 1.0, 2.0):
                # two values one unit apart: every kept column weighs at least e^-2 / V of the row, far above 4 cdf_bounds,
                # so the first and the last column of positive weight own intervals that u = 0 and u -> 1 fall well inside
                x = rs.randint(0, 2, (3, v)).astype(dtype)
                if holes and v > 2:                            # -inf at both ends and in between: never chosen
                    x[:, rs.rand(v) < 0.3] = -np.inf
                    x[:, 0] = x[:, -1] = -np.inf
                    x[:, v // 2] = 1.0
                for u in (0.0, one):
                    check_sample(x, temperature, top_k, dtype, rs, "V %d top_k %s T %g holes %s u %r" % (v, top_k, temperature, holes, u), u=u)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(do.SAMPLE_CASES))
def test_sampling_the_fixtures_cases(golden, name, dtype):
    tn.set_default_float(dtype)
    x, temperature, top_k = do.sample_case(name, np.float32)
    u = golden["sample.%s.u" % name]
    res = do.sample_reference(x, temperature, top_k, dtype)
    assert (res.margins(u) > do.MARGIN).all()
    for route in ("native", "composed"):
        assert np.array_equal(ds.run_sample(route, x, u, temperature, top_k, dtype), golden["sample.%s.ids" % name]), route


# ---------------------------------------------------------------------- end to end
@pytest.mark.parametrize("dtype", DTYPES)
def test_generation_equals_the_fixture(golden, dtype):
    """Greedy generation with the cache on the native kernels gives the fixture's tokens, and so does cache=False."""
    tn.set_default_float(dtype)
    net = ds.lm_net(golden, True, dtype)
    prompt = do.lm_prompt()
    cached = gen.generate(net, prompt, do.LM_NEW, temperature=0.0)
    assert cached.dtype == np.int64 and np.array_equal(cached, golden["lm.ids"])
    assert np.array_equal(gen.generate(net, prompt, do.LM_NEW, temperature=0.0, cache=False), cached)
    assert net.get_phase() == "TRAIN"


def test_sampled_generation_with_and_without_the_cache_agree():
    """Temperature and top-k through both routes of the token loop: the same u, the same tokens (float64: the two routes'
    logits differ in the last bits only, far below the distance of a drawn u from an interval's end)."""
    tn.set_default_float(np.float64)
    net = ds.lm_net(ds.load_golden(), True, np.float64)
    prompt = do.lm_prompt()
    a = gen.generate(net, prompt, do.LM_NEW, temperature=0.7, top_k=3, seed=5)
    b = gen.generate(net, prompt, do.LM_NEW, temperature=0.7, top_k=3, seed=5, cache=False)
    assert np.array_equal(a, b) and np.array_equal(a[:, :do.LM_PROMPT], prompt)

"""csrc/tnn_ragged.hip on the MI355X.  Decode attention with per-sequence lengths is pinned by BIT-EQUALITY with the uniform
kernel: for every sequence the result equals tnn_decode_attn on that sequence's batch slice with len = lens[b] and
splits = min(splits, chunks_b) — plus the oracle's bound, the appended rows bit for bit, nothing else written, NaN beyond
every sequence's own live prefix never read, identical bits on a repeated call.  The advance against an independent numpy
model, the embedding bit for bit, then generation: ragged prompts against float64 generations of every sequence alone,
uniform lengths against today's generate, and the captured step against the eager one.

Shapes are the smallest at which a path can go wrong: a cache of 4 chunks with lengths on both sides of every chunk edge under
every grid of 1 .. 4 workgroups (a sequence of one key then leaves three workgroups without keys), head dimensions on both
sides of the 16-byte pack and of the 64 columns one lane group covers, and 301 chunks under the clamp of 256 workgroups."""

import numpy as np
import pytest

import attn_oracle as ao
import decode_oracle as do
import decode_support as ds
import ragged_support as rs
import tinynn_autograd_amd as tn
from norm_support import dev
from tinynn_autograd_amd import decoding as dc, device_array as da, generation as gen, ragged as rg, rng

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
TMAX = 200
NEW = do.LM_NEW


@pytest.fixture(scope="module")
def golden():
    return ds.load_golden()


@pytest.fixture(scope="module")
def alone(golden):
    return rs.lm_alone(golden, do.lm_prompt(), rs.PROMPT_LENS, NEW)


def check_ragged(case, lens, dtype, splits, unaligned=False, what=""):
    tn.set_default_float(dtype)
    layout = case["layout"]
    tmax = case["k_cache"].shape[1 if layout == "bthd" else 2]
    plan = rg.plan_ragged_decode(case["q"].shape, case["k_cache"].shape, case["v_cache"].shape, (len(lens),), layout=layout,
                                 splits=splits)
    o, kc, vc = rs.run_ragged("native", case, lens, dtype, splits, unaligned)
    assert o.dtype == dtype and np.isfinite(o).all(), what                      # (NaN beyond a live prefix was never read)
    for b, n in enumerate(lens):
        if not 0 <= n < tmax:
            assert not o[b].any(), "%s: sequence %d has no valid length, zeros expected" % (what, b)
            continue
        one = rs.slice_case(case, b, n)
        eff = rg.effective_splits(n, plan.splits)
        ob, _, _ = ds.run_decode("native", one, dtype, eff, unaligned)
        assert np.array_equal(ds.bits(o[b:b + 1]), ds.bits(ob)), "%s: sequence %d (len %d, %d of %d splits) differs from " \
            "the uniform kernel by %.3e" % (what, b, n, eff, plan.splits, np.abs(o[b:b + 1] - ob).max())
        res = ds.reference(one, dtype, eff)
        ao.assert_within(o[b:b + 1], res.values["o"], res.bounds["o"], "%s sequence %d" % (what, b))
    want_k, want_v = rs.expected_ragged_caches(case, lens, dtype)
    assert np.array_equal(ds.bits(kc), ds.bits(want_k)) and np.array_equal(ds.bits(vc), ds.bits(want_v)), what
    o2, _, _ = rs.run_ragged("native", case, lens, dtype, splits, unaligned)
    assert np.array_equal(ds.bits(o), ds.bits(o2)), "%s: a repeated call gives other bits" % what
    return plan


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splits", [1, 2, 3, 4])
def test_lengths_around_the_chunk_under_every_grid(splits, dtype):
    """4 chunks; lens 0 under 4 workgroups leaves three of them without keys, 129 gives runs of unequal length under 2."""
    for lens in ((0, 64, 199), (63, 65, 129), (199, 0, 65)):
        for layout in dc.LAYOUTS:
            case = rs.ragged_case(do.case_seed("ragged%s%s" % (lens, layout)), layout, 3, 1, TMAX, 16, 24, dtype)
            plan = check_ragged(case, lens, dtype, splits, what="lens %s splits %d %s" % (lens, splits, layout))
            assert plan.chunks == 4 and plan.splits == splits
    with pytest.raises(ValueError, match="splits 5 outside"):
        rs.run_ragged("native", case, lens, dtype, 5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_sequences_of_three_heads_and_the_planners_split(dtype):
    for layout in dc.LAYOUTS:
        case = rs.ragged_case(do.case_seed("ragged23" + layout), layout, 2, 3, TMAX, 16, 24, dtype)
        for splits in (None, 3):
            plan = check_ragged(case, (129, 63), dtype, splits, what="B 2 H 3 %s splits %s" % (layout, splits))
            assert plan.splits == (4 if splits is None else 3)                  # choose_splits(6, 4): every chunk its own


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,dv", [(3, 5), (16, 4), (65, 64), (128, 65)])
def test_head_dimensions(d, dv, dtype):
    """Element accesses with one pack per lane (3 / 5), wide accesses (16 / 4), two packs per lane beyond 64 columns."""
    for layout in dc.LAYOUTS:
        case = rs.ragged_case(do.case_seed("rdims%d.%d%s" % (d, dv, layout)), layout, 3, 1, TMAX, d, dv, dtype)
        check_ragged(case, (65, 199, 0), dtype, 3, what="D %d Dv %d %s" % (d, dv, layout))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", dc.LAYOUTS)
def test_element_aligned_bases(layout, dtype):
    case = rs.ragged_case(do.case_seed("runaligned" + layout), layout, 3, 1, TMAX, 16, 8, dtype)
    check_ragged(case, (129, 0, 64), dtype, 2, unaligned=True, what="unaligned %s" % layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splits", [1, 4])
def test_the_kernel_guards_itself(splits, dtype):
    """The host cannot see lens: -1 and Tmax give zeros and untouched caches, the sequence between them its result."""
    for layout in dc.LAYOUTS:
        case = rs.ragged_case(do.case_seed("rguard" + layout), layout, 3, 2, TMAX, 16, 24, dtype)
        check_ragged(case, (-1, 70, TMAX), dtype, splits, what="guard %s splits %d" % (layout, splits))


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_chunks_than_splits_allowed(dtype):
    """301 chunks: the grid is clamped at 256 workgroups per (b, h); the sequence of 11 keys leaves 255 of its without keys
    and the combine skips their records."""
    case = rs.ragged_case(do.case_seed("rclamp"), "bhtd", 2, 1, 64 * 301, 4, 8, dtype)
    plan = check_ragged(case, (64 * 300 + 5, 10), dtype, None, what="301 chunks")
    assert plan.chunks == 301 and plan.splits == dc.MAX_SPLITS
    assert len(rg.live_runs(1, plan.splits)) == 1


def test_the_library_refuses_what_the_planner_refuses():
    from tinynn_autograd_amd import _lib
    lib = _lib.get()
    q, k, v, o = (tn.zeros(s, np.float32) for s in ((1, 1, 4), (1, 128, 1, 4), (1, 128, 1, 4), (1, 1, 4)))
    lens = tn.asarray(np.array([3], dtype=np.int64))
    ws = tn.zeros((64,), np.float32)
    strides = da._i64arr((4, 4, 0) * 3 + (512, 4, 4) * 2 + (4, 4, 0))
    for splits, v_new, msg in ((0, q, "splits 0 outside"), (3, q, r"splits 3 outside \[1, 2\]"), (1, None, "are required")):
        with pytest.raises(_lib.TnnError, match=msg):
            lib.ragged_decode_attn(q._ptr, q._ptr, None if v_new is None else v_new._ptr, k._ptr, v._ptr, o._ptr, ws._ptr, 256,
                                   lens._ptr, 1, 1, 128, 4, 4, strides, 0.5, splits, 0)


# ---------------------------------------------------------------------- the advance
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3, 257])
def test_advance_follows_the_numpy_model(B, dtype):
    """Five steps (257 sequences: two workgroups): an end of sequence on the first token, L running past Tout, no eos at all,
    the copy of the next step's u row."""
    tn.set_default_float(dtype)                                # (asarray keeps u in the operand dtype)
    Tout, N, pad = 7, 5, 9
    r = np.random.RandomState(do.case_seed("advance%d" % B))
    for eos in (2, None):
        start = r.randint(1, Tout + 1, B).astype(np.int64)
        start[0] = 4
        state = dict(lens=start - 1, start=start, done=np.zeros(B, np.int64), out=np.full((B, Tout), pad, np.int64),
                     cur=np.zeros(B, np.int64), u_all=r.random_sample((N, B)).astype(dtype), u_cur=np.zeros(B, dtype))
        lens = da.lengths(state["lens"])
        d = {k: tn.asarray(v, dtype=v.dtype) for k, v in state.items() if k != "lens"}
        assert d["u_all"].dtype == dtype and d["u_cur"].dtype == dtype
        for step in range(5):
            picked = r.randint(0, 5, B).astype(np.int64)
            if step == 0:
                picked[0] = 2                                  # sequence 0 ends on its first token (when 2 is the eos)
            state = rs.advance_model(state, picked, -1 if eos is None else eos, pad)
            da.ragged_advance(tn.asarray(picked), lens, d["start"], d["done"], d["out"], d["cur"], d["u_all"], d["u_cur"],
                              eos=eos, pad=pad, route="native")
            assert np.array_equal(lens.host, state["lens"]) and np.array_equal(np.asarray(lens.dev), state["lens"]), step
            for k in ("done", "out", "cur", "u_cur"):
                assert np.array_equal(np.asarray(d[k]), state[k]), (step, k, eos)
        assert (state["lens"] >= Tout).any() and bool(state["done"].any()) == (eos is not None)
        assert eos is None or state["out"][0].tolist() == [pad] * 4 + [2, pad, pad]
    # without u: nothing but the integers
    done, out, cur = tn.zeros((B,), np.int64), tn.zeros((B, Tout), np.int64), tn.zeros((B,), np.int64)
    lens = da.lengths(np.zeros(B, np.int64))
    da.ragged_advance(tn.asarray(np.full(B, 3, np.int64)), lens, tn.asarray(start), done, out, cur, route="native")
    assert np.asarray(out)[:, 1].tolist() == [3] * B and np.asarray(cur).tolist() == [3] * B and not np.asarray(done).any()


# ---------------------------------------------------------------------- the embedding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("E", [1, 4, 5, 16])
def test_embedding_at_bit_for_bit(E, unaligned, dtype):
    tn.set_default_float(dtype)
    r = np.random.RandomState(do.case_seed("embed_at%d" % E))
    V, Tpos, M = 11, 9, 300                                    # (300 rows of 16 columns: more than one workgroup)
    table, pos = r.randn(V, E).astype(dtype), r.randn(Tpos, E).astype(dtype)
    ids, at = r.randint(0, V, M).astype(np.int64), r.randint(0, Tpos, M).astype(np.int64)
    ids[[3, 17]], at[[5, 17]] = (-1, V), (Tpos, -2)            # out of range: a zero token row / a zero position row
    tok = np.where(((ids >= 0) & (ids < V))[:, None], table[np.clip(ids, 0, V - 1)], 0).astype(dtype)
    add = np.where(((at >= 0) & (at < Tpos))[:, None], pos[np.clip(at, 0, Tpos - 1)], 0).astype(dtype)
    td, pd = dev(table, dtype, unaligned), dev(pos, dtype, unaligned)
    got = np.asarray(da.embedding_at(td, tn.asarray(ids), tn.asarray(at), pd, route="native"))
    assert got.dtype == dtype and np.array_equal(ds.bits(got), ds.bits(tok + add))
    assert np.array_equal(got[17], np.zeros(E, dtype)) and np.array_equal(got[3], pos[at[3]]) and np.array_equal(got[5], table[ids[5]])
    none = np.asarray(da.embedding_at(td, tn.asarray(ids.reshape(M, 1)), da.lengths(at), None, route="native"))
    assert none.shape == (M, 1, E) and np.array_equal(ds.bits(none[:, 0]), ds.bits(tok))


# ---------------------------------------------------------------------- generation
@pytest.mark.parametrize("dtype", DTYPES)
def test_generate_ragged_equals_every_sequence_alone(golden, alone, dtype):
    for _, steps in alone:
        assert do.top2_margin(steps) > do.MARGIN * float(golden["lm.logit_bound"])
    tn.set_default_float(dtype)
    net = ds.lm_net(golden, True, dtype)
    prompt = do.lm_prompt()
    want, want_len = rs.expected_ids(alone, rs.PROMPT_LENS, prompt.shape[1], NEW)
    out, lengths = gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, return_lengths=True)
    assert out.dtype == np.int64 and np.array_equal(out, want) and np.array_equal(lengths, want_len)
    garbage = np.array(prompt)
    garbage[1, 2:], garbage[2, 3:] = 9, 7
    assert np.array_equal(gen.generate(net, garbage, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS), want)
    assert np.array_equal(gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, cache=False), want)
    assert np.array_equal(gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, capture=True), want)
    assert net.get_phase() == "TRAIN"


def test_generate_with_an_end_of_sequence_token(golden, alone):
    tn.set_default_float(np.float32)
    net = ds.lm_net(golden, True, np.float32)
    prompt = do.lm_prompt()
    want, want_len = rs.expected_ids(alone, rs.PROMPT_LENS, prompt.shape[1], NEW, rs.EOS, rs.PAD)
    assert want_len.tolist() == [5, 5, 11]
    kwargs = dict(temperature=0.0, prompt_lens=rs.PROMPT_LENS, eos_id=rs.EOS, pad_id=rs.PAD)
    for extra in (dict(), dict(cache=False), dict(capture=True)):
        out, lengths = gen.generate(net, prompt, NEW, return_lengths=True, **dict(kwargs, **extra))
        assert np.array_equal(out, want) and np.array_equal(lengths, want_len), extra
    new = [np.asarray(ids[p:]) for (ids, _), p in zip(alone, rs.PROMPT_LENS)]
    reached = [t for t in range(int(golden["lm.ids"].max()) + 1) if all(t in row for row in new)]
    kwargs["eos_id"] = reached[0]
    full = gen.generate(net, prompt, NEW, **kwargs)
    assert np.array_equal(full, rs.expected_ids(alone, rs.PROMPT_LENS, prompt.shape[1], NEW, reached[0], rs.PAD)[0])
    assert np.array_equal(gen.generate(net, prompt, NEW, stop_every=1, **kwargs), full)
    assert np.array_equal(gen.generate(net, prompt, NEW, stop_every=2, capture=True, **kwargs), full)


@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_lengths_give_todays_tokens(golden, dtype):
    """The ragged path at uniform lengths without an end of sequence: exactly the ids of the path that existed before."""
    tn.set_default_float(dtype)
    net = ds.lm_net(golden, True, dtype)
    prompt = do.lm_prompt()
    uniform = (prompt.shape[1],) * 3
    today = gen.generate(net, prompt, NEW, temperature=0.0)
    assert np.array_equal(today, golden["lm.ids"])
    assert np.array_equal(gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=uniform), today)
    if dtype == np.float64:
        u = np.random.RandomState(5).random_sample((NEW, 3))
        today = gen.generate(net, prompt, NEW, temperature=0.7, top_k=3, u=u)
        assert np.array_equal(gen.generate(net, prompt, NEW, temperature=0.7, top_k=3, u=u, prompt_lens=uniform), today)
    today = gen.generate(net, prompt, NEW, temperature=0.7, top_k=3, generator=rng.Generator(11))
    ragged = gen.generate(net, prompt, NEW, temperature=0.7, top_k=3, generator=rng.Generator(11), prompt_lens=uniform)
    assert np.array_equal(ragged, today)


def test_the_captured_step_gives_the_eager_ids_when_sampling(golden):
    """temperature 0.7, top_k 3, u filled by a seeded generator, ragged prompts: eager and captured runs read the same u rows."""
    tn.set_default_float(np.float64)
    net = ds.lm_net(golden, True, np.float64)
    prompt = do.lm_prompt()
    kwargs = dict(temperature=0.7, top_k=3, prompt_lens=rs.PROMPT_LENS)
    eager = gen.generate(net, prompt, NEW, generator=rng.Generator(11), **kwargs)
    assert np.array_equal(gen.generate(net, prompt, NEW, generator=rng.Generator(11), capture=True, **kwargs), eager)
    assert not np.array_equal(gen.generate(net, prompt, NEW, generator=rng.Generator(12), **kwargs), eager)

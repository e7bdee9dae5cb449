"""The ragged decoding step on the CPU test twin, where everything takes the composed route: the planner and its split rule,
the composed decode attention per sequence within the oracle's bounds, the step's bookkeeping against an independent numpy
model, and generate() on ragged prompts, with an end-of-sequence token, without the cache and with stop_every, against float64
generations of every sequence ALONE."""

import numpy as np
import pytest

import attn_oracle as ao
import decode_oracle as do
import decode_support as ds
import ragged_support as rs
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import decoding as dc, device_array as da, generation as gen, ragged as rg
from tinynn_autograd_amd.core import ops
from tinynn_autograd_amd.core.layers import Embedding
from tinynn_autograd_amd.core.tensor import Tensor

NEW = do.LM_NEW


@pytest.fixture(scope="module")
def golden():
    return ds.load_golden()


@pytest.fixture(scope="module")
def alone(golden):
    """Computed once: every sequence of the ragged prompt generated alone in float64."""
    return rs.lm_alone(golden, do.lm_prompt(), rs.PROMPT_LENS, NEW)


@pytest.fixture(autouse=True)
def _switches():
    yield
    da.DECODE_ROUTE = None
    da.RAGGED_ROUTE = None


def test_planner_validation():
    ok = dict(q_shape=(2, 3, 8), k_cache_shape=(2, 200, 3, 8), v_cache_shape=(2, 200, 3, 5), lens_shape=(2,))
    p = rg.plan_ragged_decode(**ok)
    assert (p.B, p.H, p.D, p.Dv, p.Tmax, p.chunks) == (2, 3, 8, 5, 200, 4) and p.out_shape == (2, 3, 5) and p.route == "native"
    assert p.geometry() == (2, 3, 200, 8, 5)
    assert p.strides() == dc.plan_decode(ok["q_shape"], ok["k_cache_shape"], ok["v_cache_shape"], 7).strides()
    assert p.workspace_bytes(4) == dc._round16(2 * 3 * p.splits * 7 * 4)
    assert rg.plan_ragged_decode(native=False, **ok).route == "composed"
    assert rg.plan_ragged_decode(float_ok=False, **ok).route == "composed"
    for bad, match in ((dict(lens_shape=(3,)), "one length per sequence"), (dict(lens_shape=(2, 1)), "one length per sequence"),
                       (dict(q_shape=(2, 3)), r"q must be \[B, H, D\]"), (dict(v_cache_shape=(2, 100, 3, 5)), "does not match"),
                       (dict(k_new_shape=(2, 3, 9)), "k_new must be"), (dict(splits=0), "splits 0 outside"),
                       (dict(splits=5), r"splits 5 outside \[1, 4\]"), (dict(route="fwd"), "route must be one of"),
                       (dict(layout="tbhd"), "layout must be one of")):
        with pytest.raises(ValueError, match=match) as err:
            rg.plan_ragged_decode(**dict(ok, **bad))
        assert "attention_decode:" not in str(err.value)
    with pytest.raises(ValueError, match="native ragged decode attention route"):
        rg.plan_ragged_decode(native=False, route="native", **ok)
    assert rg.plan_ragged_decode(splits=4, **ok).splits == 4


def test_the_split_depends_on_shapes_alone_and_reproduces_the_uniform_split():
    """splits = choose_splits(B H, ceil(Tmax / CHUNK)); the workgroups of a sequence that get keys are exactly the runs of
    min(splits, chunks_b) splits, in order — at uniform lengths that is the split plan_decode picks at every step."""
    for b, h, tmax in ((1, 1, 64), (1, 2, 200), (2, 4, 4096), (8, 8, 700), (1, 1, 64 * 301), (64, 16, 300)):
        shapes = ((b, h, 8), (b, tmax, h, 8), (b, tmax, h, 8))
        p = rg.plan_ragged_decode(*shapes, lens_shape=(b,))
        chunks = -(-tmax // dc.CHUNK)
        assert p.splits == dc.choose_splits(b * h, chunks) and 1 <= p.splits <= min(chunks, dc.MAX_SPLITS)
        for length in sorted({0, 1, 63, 64, 65, tmax // 2, tmax - 2, tmax - 1}):
            if 0 <= length < tmax:
                uniform = dc.plan_decode(*shapes, length)
                assert rg.effective_splits(length, p.splits) == uniform.splits, (b, h, tmax, length)
                assert rg.live_runs(uniform.chunks, p.splits) == uniform.runs(), (b, h, tmax, length)
    for c in range(1, 40):                                     # the claim itself, beyond what a planner would pick
        for s in list(range(1, 70)) + [128, 255, 256, 299]:
            want = [(i * c // min(s, c), (i + 1) * c // min(s, c)) for i in range(min(s, c))]
            assert rg.live_runs(c, s) == want, (c, s)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["bthd", "bhtd"])
def test_composed_attention_per_sequence_within_the_bounds(layout, dtype):
    tn.set_default_float(dtype)
    lens = (0, 129, 70)
    case = rs.ragged_case(11, layout, 3, 2, 140, 16, 5, np.float32)
    o, kc, vc = rs.run_ragged("composed", case, lens, dtype)
    assert o.dtype == dtype and o.shape == (3, 2, 5) and np.isfinite(o).all()
    for b, n in enumerate(lens):
        res = ds.reference(rs.slice_case(case, b, n), dtype, 1)
        ao.assert_within(o[b:b + 1], res.values["o"], res.bounds["o"], "sequence %d" % b)
    want_k, want_v = rs.expected_ragged_caches(case, lens, dtype)
    assert np.array_equal(ds.bits(kc), ds.bits(want_k)) and np.array_equal(ds.bits(vc), ds.bits(want_v))
    # the guard: no such row -> zeros, the caches untouched
    lens = (-1, 70, 140)
    o, kc, vc = rs.run_ragged("composed", case, lens, dtype)
    assert not o[0].any() and not o[2].any() and np.isfinite(o[1]).all() and o[1].any()
    want_k, want_v = rs.expected_ragged_caches(case, lens, dtype)
    assert np.array_equal(ds.bits(kc), ds.bits(want_k)) and np.array_equal(ds.bits(vc), ds.bits(want_v))


def test_ops_give_leaves_and_refuse_unknown_arguments():
    case = rs.ragged_case(3, "bthd", 2, 3, 96, 16, 24, np.float32)
    q, kn, vn = (Tensor(case[n], requires_grad=True) for n in ("q", "k_new", "v_new"))
    kc, vc = tn.asarray(case["k_cache"]), tn.asarray(case["v_cache"])
    lens = da.lengths([70, 5])
    out = ops.attention_decode_ragged_(q, kc, vc, lens, kn, vn)
    assert not out.requires_grad and out.dependency == [] and tuple(out.shape) == (2, 3, 24)
    table = Tensor(np.arange(12, dtype=np.float32).reshape(4, 3), requires_grad=True)
    emb = ops.embedding_at_(table, tn.asarray(np.array([[1], [3]])), lens)
    assert not emb.requires_grad and emb.dependency == [] and np.asarray(emb.values).tolist() == [[[3, 4, 5]], [[9, 10, 11]]]
    for call in (lambda: ops.attention_decode_ragged_(q, kc, vc, lens, kn, vn, causal=True),
                 lambda: ops.embedding_at_(table, tn.asarray(np.array([1])), lens, padding_idx=0)):
        with pytest.raises(TypeError, match="unsupported arguments"):
            call()
    with pytest.raises(ValueError, match="k_new and v_new are required"):
        da.attention_decode_ragged(q.values, kc, vc, lens, None, None)
    with pytest.raises(TypeError, match="dense int64 device array"):
        da.attention_decode_ragged(q.values, kc, vc, np.array([70, 5]), kn.values, vn.values)


def test_advance_follows_the_numpy_model():
    """Five steps of B = 3: an end of sequence on the first token, L running past Tout, the copy of the next u row."""
    B, Tout, N, eos, pad = 3, 7, 5, 2, 9
    r = np.random.RandomState(5)
    start = np.array([4, 1, 6], dtype=np.int64)
    state = dict(lens=start - 1, start=start, done=np.zeros(B, np.int64), out=np.full((B, Tout), pad, np.int64),
                 cur=np.zeros(B, np.int64), u_all=r.random_sample((N, B)).astype(np.float32), u_cur=np.zeros(B, np.float32))
    lens = da.lengths(state["lens"])
    d = {k: tn.asarray(v) for k, v in state.items() if k != "lens"}
    picks = [np.array([2, 3, 4]), np.array([7, 2, 1]), np.array([7, 7, 7]), np.array([1, 1, 2]), np.array([3, 3, 3])]
    for step, picked in enumerate(picks):
        state = rs.advance_model(state, picked, eos, pad)
        da.ragged_advance(tn.asarray(picked), lens, d["start"], d["done"], d["out"], d["cur"], d["u_all"], d["u_cur"], eos=eos, pad=pad)
        assert np.array_equal(lens.host, state["lens"]) and np.array_equal(np.asarray(lens.dev), state["lens"]), step
        for k in ("done", "out", "cur", "u_cur"):
            assert np.array_equal(np.asarray(d[k]), state[k]), (step, k)
    assert state["done"].tolist() == [1, 1, 1] and state["out"][0].tolist() == [9, 9, 9, 9, 2, 9, 9]
    assert state["lens"].tolist() == [8, 5, 10]                # sequences 0 and 2 ran past Tout: nothing written there
    # eos None: nobody ends; no u at all
    done, out, cur = tn.asarray(np.zeros(B, np.int64)), tn.asarray(np.zeros((B, Tout), np.int64)), tn.asarray(np.zeros(B, np.int64))
    lens = da.lengths([0, 1, 2])
    da.ragged_advance(tn.asarray(np.array([2, 2, 2])), lens, tn.asarray(start), done, out, cur)
    assert not np.asarray(done).any() and np.asarray(cur).tolist() == [2, 2, 2] and lens.host.tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="come together"):
        da.ragged_advance(cur, lens, tn.asarray(start), done, out, cur, u_all=d["u_all"])
    with pytest.raises(ValueError, match="picked must have shape"):
        da.ragged_advance(tn.asarray(np.array([1, 2])), lens, tn.asarray(start), done, out, cur)


def test_embedding_positions():
    r = np.random.RandomState(3)
    layer = Embedding(7, 4, max_len=6)
    ids = r.randint(0, 7, (3, 6))
    whole = np.asarray(layer.forward(Tensor(ids)).values)
    at = (5, 0, 2)
    one = np.stack([ids[b, t] for b, t in enumerate(at)]).reshape(3, 1)
    got = np.asarray(layer.forward(Tensor(tn.asarray(one)), positions=da.lengths(at)).values)
    assert got.shape == (3, 1, 4)
    assert np.array_equal(got[:, 0], np.stack([whole[b, t] for b, t in enumerate(at)]))       # bit for bit: the same rows added
    with pytest.raises(ValueError, match="outside max_len 6"):
        layer.forward(Tensor(tn.asarray(one)), positions=da.lengths((5, 6, 2)))
    with pytest.raises(ValueError, match="excludes `offset`"):
        layer.forward(Tensor(tn.asarray(one)), offset=1, positions=da.lengths(at))
    with pytest.raises(ValueError, match="one position per sequence"):
        layer.forward(Tensor(tn.asarray(ids)), positions=da.lengths(at))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_generate_ragged_equals_every_sequence_alone(golden, alone, dtype):
    """Prompt lengths (4, 2, 3), 8 new tokens, greedy: row by row the float64 generation of that sequence alone.  The inputs
    qualify: the top-2 margin of every step exceeds MARGIN logit bounds, so no path within the bound can change a token."""
    for _, steps in alone:
        assert do.top2_margin(steps) > do.MARGIN * float(golden["lm.logit_bound"])
    tn.set_default_float(dtype)
    net = ds.lm_net(golden, True, dtype)
    prompt = do.lm_prompt()
    want, want_len = rs.expected_ids(alone, rs.PROMPT_LENS, prompt.shape[1], NEW)
    out, lengths = gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, return_lengths=True)
    assert out.dtype == np.int64 and out.shape == (3, 12) and np.array_equal(out, want)
    assert np.array_equal(lengths, want_len) and lengths.tolist() == [12, 10, 11]
    assert net.get_phase() == "TRAIN"
    # what the prompt holds beyond P_b does not matter
    garbage = np.array(prompt)
    garbage[1, 2:], garbage[2, 3:] = 9, 7
    assert np.array_equal(gen.generate(net, garbage, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS), want)
    # the independent route: the whole growing prefix every step
    assert np.array_equal(gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, cache=False), want)
    # prompt_lens None on the ragged path: every sequence has Pmax tokens -> the fixture's tokens
    same, lengths = gen.generate(net, prompt, NEW, temperature=0.0, return_lengths=True)
    assert np.array_equal(same, golden["lm.ids"]) and lengths.tolist() == [12, 12, 12]


def test_generate_with_an_end_of_sequence_token(golden, alone):
    tn.set_default_float(np.float32)
    net = ds.lm_net(golden, True, np.float32)
    prompt = do.lm_prompt()
    new = [np.asarray(ids[p:]) for (ids, _), p in zip(alone, rs.PROMPT_LENS)]
    assert new[0][0] == rs.EOS and new[1][2] == rs.EOS and rs.EOS not in new[1][:2] and rs.EOS not in new[2]   # the fixture
    assert all(rs.PAD not in row for row in new)
    want, want_len = rs.expected_ids(alone, rs.PROMPT_LENS, prompt.shape[1], NEW, rs.EOS, rs.PAD)
    assert want_len.tolist() == [5, 5, 11]
    for cache in (True, False):
        out, lengths = gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, eos_id=rs.EOS, pad_id=rs.PAD,
                                    return_lengths=True, cache=cache)
        assert np.array_equal(out, want) and np.array_equal(lengths, want_len), "cache=%s" % cache
    assert out[0].tolist() == list(prompt[0]) + [rs.EOS] + [rs.PAD] * 7
    assert out[1, 5:].tolist() == [rs.PAD] * 7 and out[2, 11] == rs.PAD
    # an end of sequence that every sequence reaches: stop_every=1 leaves early and returns the same ids
    ends = [int(row[-1]) for row in new]
    reached = [t for t in range(int(golden["lm.ids"].max()) + 1) if all(t in row for row in new)]
    assert reached, "the fixture's generations share no token: %s" % ends
    full = gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, eos_id=reached[0], pad_id=rs.PAD)
    early = gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, eos_id=reached[0], pad_id=rs.PAD,
                         stop_every=1)
    assert np.array_equal(full, early)
    assert np.array_equal(full, rs.expected_ids(alone, rs.PROMPT_LENS, prompt.shape[1], NEW, reached[0], rs.PAD)[0])


def test_generate_ragged_arguments(golden):
    net = ds.lm_net(golden, True, np.float32)
    prompt = do.lm_prompt()
    with pytest.raises(ValueError, match="capture=True needs the native route"):
        gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=rs.PROMPT_LENS, capture=True)
    with pytest.raises(ValueError, match="needs cache=True"):
        gen.generate(net, prompt, NEW, temperature=0.0, capture=True, cache=False)
    for bad in ((4, 2), (4, 0, 3), (4, 5, 3), (4.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="prompt_lens must be"):
            gen.generate(net, prompt, NEW, temperature=0.0, prompt_lens=bad)
    with pytest.raises(ValueError, match="stop_every must be"):
        gen.generate(net, prompt, NEW, temperature=0.0, stop_every=0)
    with pytest.raises(ValueError, match="exceed the embedding's max_len 12"):
        gen.generate(net, prompt, NEW + 1, temperature=0.0, prompt_lens=rs.PROMPT_LENS)
    out, lengths = gen.generate(net, prompt, 0, prompt_lens=rs.PROMPT_LENS, pad_id=rs.PAD, return_lengths=True)
    assert out.shape == (3, 4) and out[1].tolist() == list(prompt[1, :2]) + [rs.PAD] * 2 and lengths.tolist() == [4, 2, 3]
    # sampling: the same u gives the tokens of the uniform path at uniform lengths
    u = np.random.RandomState(7).random_sample((3, 3))
    assert np.array_equal(gen.generate(net, prompt, 3, temperature=0.8, top_k=4, u=u, eos_id=99),
                          gen.generate(net, prompt, 3, temperature=0.8, top_k=4, u=u))
    assert net.get_phase() == "TRAIN"


def test_example_generates_ragged():
    """examples/charlm_run.py --generate N --ragged --eos ID: prompts of differing lengths, ids in range, rows padded after
    an end of sequence."""
    import token_support as ts
    example = ts.load_example()
    args = example.parse(["--n_train", "64", "--n_test", "8", "--num_ep", "1", "--batch_size", "32", "--generate", "4",
                          "--ragged", "--eos", "3"])
    history = example.main(args)
    generated, share = args.generation
    assert len(history) == 1 and generated.shape == (8, 2 * 4 + 4) and generated.dtype == np.int64
    assert ((generated >= 0) & (generated < 16)).all() and 0.0 <= share <= 1.0
    lens = 4 + np.arange(8) % 5
    for b, p in enumerate(lens):
        new = generated[b, p:p + 4]
        hit = np.nonzero(new == 3)[0]
        assert not hit.size or not new[hit[0] + 1:].any()                          # pad 0 after the end of sequence
        assert not generated[b, p + 4:].any()                                      # trailing pads

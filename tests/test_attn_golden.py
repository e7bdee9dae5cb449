"""tests/golden/attn_cases.npz: the float64 oracle still reproduces it (operands rebuilt from the seeds), and the composed
route — the one the session's backend can always run — stays inside the derived bounds on every case, float32 and float64."""

import os

import numpy as np
import pytest

import attn_oracle as ao
import tinynn_autograd_amd as tn
from tinynn_autograd_amd import device_array as da

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_cases.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as data:
        return dict(data)


def test_fixture_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert sorted(golden) == sorted("%s.%s" % (n, f) for n in ao.ATTN_CASES for f in ao.FIELDS)


def test_oracle_reproduces_the_fixture(golden):
    for name in ao.ATTN_CASES:
        q, k, v, do, causal, scale, layout = ao.case_input(name)
        res = ao.reference(q, k, v, do, causal, scale, layout)
        for field in ao.FIELDS:
            np.testing.assert_allclose(res.values[field], golden["%s.%s" % (name, field)], rtol=1e-13, atol=1e-300,
                                       err_msg="%s %s" % (name, field))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_composed_route_within_the_bounds(golden, dtype):
    for name in ao.ATTN_CASES:
        q, k, v, do, causal, scale, layout = ao.case_input(name)
        res = ao.reference(q, k, v, do, causal, scale, layout, dtype)
        for field in ao.FIELDS:
            res.values[field] = golden["%s.%s" % (name, field)]
        qd, kd, vd, dod = (tn.asarray(a, dtype=dtype) for a in (q, k, v, do))
        opts = dict(causal=causal, scale=scale, layout=layout, route="composed")
        o, lse = da.attention(qd, kd, vd, **opts)
        dq, delta = da.attention_bwd_q(qd, kd, vd, o, dod, lse, **opts)
        dk, dv = da.attention_bwd_kv(qd, kd, vd, dod, lse, delta, **opts)
        assert o.dtype == dtype and lse.dtype == dtype
        ao.check(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv), res, "%s %s" % (name, np.dtype(dtype).name))

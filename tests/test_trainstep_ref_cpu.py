"""The condition that makes the bars of tests/test_trainstep_parity.py meaningful, checked without a GPU: for every step those
tests run, the fp32 oracle (oracle.train_step) and the float64 restatement with the oracle's discrete decisions
(tests/trainstep_ref.py) agree in the six loss values to 1e-5 and in each gradient block (v, q, t) to 5e-5 -- the oracle's own
rounding noise uses at most half of the 1e-4 the kernel is held to.  A batch seed that does not meet this is replaced; the
bar is not widened."""
import pytest
import torch

from conftest import rel_err
import trainstep_ref as R
from oracle import vpn_oracle as O


@pytest.mark.parametrize('step_id', R.STEP_IDS)
def test_oracle_within_half_the_bar_of_float64(step_id):
    _, case, _, w, _ = R.STEP_BY_ID[step_id]
    l32, g32, l64, g64 = R.references(step_id)
    print(step_id, 'losses', (l32.double() - l64).abs().max().item())
    assert torch.allclose(l32.double(), l64, rtol=1e-5, atol=1e-8), (l32, l64)
    zero = R.zero_blocks(w)
    for name, sl in R.BLOCKS:
        if name in zero:                                       # must be zero identically, not to rounding
            assert int(torch.count_nonzero(g32[..., sl])) == 0 and int(torch.count_nonzero(g64[..., sl])) == 0, name
            continue
        assert float(g64[..., sl].abs().max()) > 0, name
        e = rel_err(g32[..., sl], g64[..., sl])
        print(step_id, name, 'rel_err fp32 oracle vs float64: %.2e' % e)
        assert e <= 5e-5, (name, e)


def test_terms_that_are_off_are_exactly_zero():
    """An isolated term leaves the other four values at exactly 0 in both references, and the total equal to the term."""
    for wn, w in R.W_ISOLATED.items():
        l32, _, l64, _ = R.references('A-mixed-%s' % wn)
        on = [i for i in range(5) if w[i]]
        assert len(on) == 1
        for l in (l32, l64):
            assert all(float(l[i]) == 0.0 for i in range(5) if i not in on), (wn, l)
            assert float(l[on[0]]) > 0 and float(l[5]) == float(l[on[0]]), (wn, l)


def test_oracle_defaults_and_keywords():
    """The keywords added to oracle.train_step: the defaults spelled out give the same bits as leaving them out, the
    losses do not depend on grad_scale and the gradient is linear in it, sample_base b draws what sample b of a larger
    batch draws."""
    B, K, n, M, Mc, H, W, _ = R.CASES['A']
    inputs = R.batch('A')
    kinds = R.kinds_of('mixed', K)
    w = (1.0, 0.7, 1.0, 0.1, 0.0)                                  # the auction is off: not what is checked here
    l0, g0 = O.train_step(*inputs, kinds, n, H, W, w, R.SEED)
    l1, g1, dec = O.train_step(*inputs, kinds, n, H, W, w, R.SEED, sample_base=0, cd_w1=1.0, cd_w2=1.0, sil_mse=False,
                               grad_scale=1.0, return_decisions=True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert dec['emd_assign'] is None and dec['face_counts'].shape == (B, K, 6)
    assert torch.equal(dec['face_counts'].sum(-1), torch.tensor([n] * (K // 2) + [0] * (K - K // 2), dtype=torch.int32).expand(B, K))
    l2, g2 = O.train_step(*inputs, kinds, n, H, W, w, R.SEED, grad_scale=-4.0)
    assert torch.equal(l2, l0) and torch.equal(g2, -4.0 * g0)      # a power of two commutes with every rounding
    one = [x[1:2] for x in inputs]
    l3, g3 = O.train_step(*one, kinds, n, H, W, w, R.SEED, sample_base=1)
    l4, g4 = O.train_step(*one, kinds, n, H, W, w, R.SEED)
    assert not torch.equal(l3, l4)
    u = O.philox_uniforms(R.SEED, 0, B, K, n)
    assert torch.equal(O.philox_uniforms(R.SEED, 1, 1, K, n)[0], u[1])

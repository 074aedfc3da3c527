"""numpy restatement of vpn_adam_step's arithmetic (include/vpn_hip.h, csrc/optim.hip), bit for bit: fp32 arrays with every
operation rounded by itself, the step's scalars formed in double from the ADVANCED products b1pow * beta1 and b2pow * beta2,
which grow by one double multiplication per step (no pow)."""
import math

import numpy as np

F = np.float32

# torch's CPU kernels round some operations differently, so the restatement and torch.optim.Adam are not
# bit-equal.  MEASURED_ULP is the worst distance of a parameter, in representable fp32 values, over the seeds, the two
# weight decays and the 20 steps of tests/test_optim_cpu.py::test_restatement_follows_torch_adam (parameters of magnitude 0.5 .. 2, so that a
# distance in ulps means 6e-8 .. 1.2e-7 relative).  The bound is four times that: rounding differences of independent steps
# add up roughly linearly, and the test guards against a wrong formula, it claims no precision.  tests/test_optim.py
# holds torch.optim.Adam on the GPU to the same bound.
MEASURED_ULP = 1
ULP_BOUND = 4 * MEASURED_ULP


class AdamRefState:
    """The device state block of a parameter group: {step, b1pow, b2pow} (arrivals is 0 between launches)."""

    def __init__(self, step=0, beta1=0.9, beta2=0.999):
        self.step, self.b1pow, self.b2pow = 0, 1.0, 1.0
        for _ in range(step):
            self.advance(beta1, beta2)

    def advance(self, beta1, beta2):
        self.step += 1
        self.b1pow *= beta1
        self.b2pow *= beta2


def adam_scalars(state, lr, beta1, beta2, eps, wd):
    B1, B2 = state.b1pow * beta1, state.b2pow * beta2
    return dict(c1=F(1.0 - beta1), c2=F(1.0 - beta2), b2f=F(beta2), wdf=F(wd), epsf=F(eps), bc2s=F(math.sqrt(1.0 - B2)),
                nss=F(-(lr / (1.0 - B1))))


def adam_update(p, g, m, v, k, wd):
    """One parameter's update with the scalars k: returns (p', m', v') as new fp32 arrays."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    with np.errstate(all='ignore'):
        g1 = g + k['wdf'] * p if wd != 0 else g
        m2 = m + k['c1'] * (g1 - m)
        v2 = v * k['b2f'] + k['c2'] * (g1 * g1)
        den = np.sqrt(v2) / k['bc2s'] + k['epsf']
        p2 = p + k['nss'] * (m2 / den)
    assert p2.dtype == F and m2.dtype == F and v2.dtype == F
    return p2, m2, v2


def adam_ref_step(params, grads, ms, vs, state, lr, beta1, beta2, eps, wd):
    """One step of a group: lists of fp32 arrays, grads[i] None = no gradient (that parameter keeps p, m, v).  `lr` is the
    double the kernel sees (float(np.float32(x)) for a device learning rate).  Advances `state` when any parameter has a
    gradient, as the kernel's last workgroup does.  Returns new lists (p, m, v)."""
    if all(g is None for g in grads):
        return list(params), list(ms), list(vs)
    k = adam_scalars(state, lr, beta1, beta2, eps, wd)
    out = [(p, m, v) if g is None else adam_update(p, g, m, v, k, wd) for p, g, m, v in zip(params, grads, ms, vs)]
    state.advance(beta1, beta2)
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def ulp_distance(a, b):
    """Largest distance between two fp32 arrays counted in representable values (finite values of either sign)."""
    a, b = np.ascontiguousarray(a, dtype=F).ravel(), np.ascontiguousarray(b, dtype=F).ravel()
    if a.size == 0:
        return 0

    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)

    return int(np.abs(ordered(a) - ordered(b)).max())

"""CPU-only checks of the optimiser stage (csrc/optim.hip, modules/optim.py): the C ABI, the host table
builder, what the constructor refuses, and the restatement tests/optim_ref.py against torch.optim.Adam."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
import optim_ref as R

ULP_BOUND = R.ULP_BOUND


def test_library_exports_the_optimiser_entry_points():
    import importlib.util
    spec = importlib.util.spec_from_file_location('vpn_build', os.path.join(ROOT, 'volumetric-primitives-net_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'optim.hip' in b.SOURCES and b.PER_FILE['optim.hip'] == ['-ffp-contract=off']
    L = ctypes.CDLL(b.build(verbose=False))
    for name in ('vpn_adam_step', 'vpn_adam_table_bytes'):
        assert hasattr(L, name), name
    import vpn_amd._lib as lib
    _v, _i = ctypes.c_void_p, ctypes.c_int
    assert lib.SIGNATURES['vpn_adam_step'] == (_i, [_v, _i, _v, _i, _v, _v, _v, _i, _v])
    assert lib.SIGNATURES['vpn_adam_table_bytes'] == (ctypes.c_size_t, [_i, ctypes.c_longlong])
    assert lib.lib().vpn_abi_version() == lib.ABI_VERSION == 9          # entries were added, none changed


def test_argument_validation_needs_no_gpu():
    import vpn_amd._lib as lib
    from vpn_amd import ops
    L = lib.lib()
    bad = lib.CONSTANTS['VPN_E_BADARG']
    hyper = (ctypes.c_double * 5)(1e-3, 0.9, 0.99, 1e-8, 0.0)
    table = (ctypes.c_longlong * 8)()          # host memory standing in for the tables: validation never reads them
    assert L.vpn_adam_step(None, 1, None, 1, None, None, None, 0, None) == bad
    assert L.vpn_adam_step(None, 1, table, 1, table, hyper, None, 0, None) == bad
    assert L.vpn_adam_step(table, 1, table, 1, None, hyper, None, 0, None) == bad
    assert L.vpn_adam_step(table, 1, table, 1, table, None, None, 0, None) == bad
    assert L.vpn_adam_step(table, 1, table, 0, table, hyper, None, 0, None) == bad
    assert L.vpn_adam_step(table, 1, table, -2, table, hyper, None, 0, None) == bad
    assert L.vpn_adam_step(table, -1, table, 1, table, hyper, None, 0, None) == bad
    for i, value in ((1, 1.0), (2, -0.1), (3, -1e-8), (4, float('nan')), (0, float('inf'))):
        h = (ctypes.c_double * 5)(1e-3, 0.9, 0.99, 1e-8, 0.0)
        h[i] = value
        assert L.vpn_adam_step(table, 1, table, 1, table, h, None, 0, None) == bad, (i, value)
    assert L.vpn_adam_step(None, 0, None, 0, None, None, None, 0, None) == 0        # zero segments: a successful no-op
    chunk = lib.CONSTANTS['VPN_ADAM_CHUNK']
    assert chunk == ops.ADAM_CHUNK and chunk % 1024 == 0 and lib.CONSTANTS['VPN_ADAM_STATE_BYTES'] == 32
    for S, n in ((0, 0), (1, 1), (3, 2 * chunk + 7), (130, 130 * 5), (92, 23_400_000)):
        assert L.vpn_adam_table_bytes(S, n) == S * 48 + 16 * (n // chunk + S), (S, n)
    assert L.vpn_adam_table_bytes(-1, 5) == 0 and L.vpn_adam_table_bytes(1, -5) == 0


def test_table_builder_rows():
    from vpn_amd import ops
    C = ops.ADAM_CHUNK
    sizes = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7, 0]
    base = 0x7f0000000000
    entries = [(base + 0x100000 * i, base + 0x100000 * i + 0x40000, base + 0x100000 * i + 0x80000, base + 0x100000 * i + 0xc0000, n)
               for i, n in enumerate(sizes)]
    entries.insert(4, (base - 0x1000, None, base - 0x2000, base - 0x3000, 77))        # a parameter without a gradient
    segments, chunks = ops.adam_tables(entries)
    assert [s[4] for s in segments] == sizes and all(s[5] == 1 for s in segments)
    assert [s[:4] for s in segments] == [e[:4] for e in entries if e[1] is not None]
    assert chunks == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (6, C), (7, 0), (7, C), (7, 2 * C)]
    assert len(chunks) == 11                                     # the empty segment keeps its row and has no chunk
    # every element of every segment is covered exactly once
    for s, (_, _, _, _, n, _) in enumerate(segments):
        firsts = [f for seg, f in chunks if seg == s]
        assert firsts == list(range(0, n, C))
    assert len(segments) * 48 + len(chunks) * 16 <= 9 * 48 + 16 * (sum(sizes) // C + 9)       # vpn_adam_table_bytes bounds it
    assert ops.adam_tables([]) == ([], []) and ops.adam_tables([(16, None, 32, 48, 5)]) == ([], [])


def test_alignment_decision_per_segment():
    """16-byte accesses only where all four pointers of the segment are 16-byte aligned."""
    from vpn_amd import ops
    a = 0x7f0000001000
    ptrs = [((a, a + 0x100, a + 0x200, a + 0x300), 1),
            ((a + 4, a + 0x100, a + 0x200, a + 0x300), 0),          # p misaligned (a view at a 4-byte offset)
            ((a, a + 0x108, a + 0x200, a + 0x300), 0),              # g misaligned by 8
            ((a, a + 0x100, a + 0x20c, a + 0x300), 0),              # m
            ((a, a + 0x100, a + 0x200, a + 0x304), 0),              # v
            ((a + 16, a + 0x110, a + 0x230, a + 0x3f0), 1)]
    segments, _ = ops.adam_tables([p + (10,) for p, _ in ptrs])
    assert [s[5] for s in segments] == [want for _, want in ptrs]


def test_constructor_refuses_what_it_cannot_run():
    import vpn_amd
    with pytest.raises(RuntimeError, match='GPU only'):
        vpn_amd.Adam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match='amsgrad'):
        vpn_amd.Adam([torch.nn.Parameter(torch.zeros(4))], amsgrad=True)
    with pytest.raises(ValueError, match='maximize'):
        vpn_amd.Adam([torch.nn.Parameter(torch.zeros(4))], maximize=True)
    with pytest.raises(ValueError, match='fp32'):
        vpn_amd.Adam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError, match='contiguous'):
        vpn_amd.Adam([torch.nn.Parameter(torch.zeros(4, 4).t()[1:])])
    with pytest.raises(ValueError, match='betas'):
        vpn_amd.Adam([torch.nn.Parameter(torch.zeros(4))], betas=(1.0, 0.99))
    assert issubclass(vpn_amd.Adam, torch.optim.Optimizer) and vpn_amd.Adam is vpn_amd.modules.optim.Adam


def test_param_group_keys_are_torchs():
    from vpn_amd.modules import optim
    d = optim._torch_adam_defaults()
    assert list(d) == list(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).param_groups[0])[1:]
    assert optim.advance_powers(0, 0.9, 0.99) == (1.0, 1.0)
    assert optim.advance_powers(3, 0.9, 0.99) == (1.0 * 0.9 * 0.9 * 0.9, 1.0 * 0.99 * 0.99 * 0.99)
    st = R.AdamRefState(3, 0.9, 0.99)
    assert (st.step, st.b1pow, st.b2pow) == (3,) + optim.advance_powers(3, 0.9, 0.99)


def _torch_run(seed, wd, steps=20, n=4099):
    """The restatement and torch.optim.Adam (CPU, fp32, foreach=False) on the same gradients, magnitudes 1e-4 .. 1e1:
    the worst parameter distance in ulps after any step, and the two final parameter vectors."""
    rng = np.random.default_rng(seed)
    p0 = (rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=1e-4, betas=(0.9, 0.99), weight_decay=wd, foreach=False)
    st = R.AdamRefState()
    p, m, v = [p0.copy()], [np.zeros(n, np.float32)], [np.zeros(n, np.float32)]
    worst = 0
    for _ in range(steps):
        g = (10.0 ** rng.uniform(-4, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adam_ref_step(p, [g], m, v, st, 1e-4, 0.9, 0.99, 1e-8, wd)
        worst = max(worst, R.ulp_distance(p[0], tp.detach().numpy()))
    assert st.step == steps
    return worst, p0, p[0], tp.detach().numpy()


@pytest.mark.parametrize('wd', [0.0, 1e-6])
def test_restatement_follows_torch_adam(wd):
    worst = 0
    for seed in range(4):
        d, p0, ours, theirs = _torch_run(seed, wd)
        print('weight_decay %g seed %d: worst parameter distance %d ulp' % (wd, seed, d))
        worst = max(worst, d)
        assert np.abs(ours - p0).max() > 2e-4                                      # 20 steps of 1e-4 did move them
    assert worst <= ULP_BOUND, worst


def test_restatement_details():
    """The parts torch cannot show: a parameter without a gradient is skipped and does not stop the group's step, a group
    without any gradient does not advance, a device learning rate is the float's value, non-finite gradients propagate."""
    st = R.AdamRefState()
    p = [np.ones(3, np.float32), np.full(2, 2.0, np.float32)]
    m = [np.zeros(3, np.float32), np.zeros(2, np.float32)]
    v = [np.zeros(3, np.float32), np.zeros(2, np.float32)]
    p1, m1, v1 = R.adam_ref_step(p, [None, None], m, v, st, 1e-3, 0.9, 0.99, 1e-8, 0.0)
    assert st.step == 0 and all(a is b for a, b in zip(p1, p))
    g = np.array([0.5, -0.25], np.float32)
    p2, m2, v2 = R.adam_ref_step(p, [None, g], m, v, st, 1e-3, 0.9, 0.99, 1e-8, 0.0)
    assert st.step == 1 and st.b1pow == 0.9 and st.b2pow == 0.99 and p2[0] is p[0]
    # the first step of Adam moves every element by lr against its gradient's sign, whatever its size (to rounding)
    np.testing.assert_allclose(p2[1], np.float32(2.0) - np.float32(1e-3) * np.sign(g), rtol=1e-6)
    np.testing.assert_array_equal(m2[1], np.float32(0.0) + np.float32(1.0 - 0.9) * g)
    bad = np.array([np.nan, np.inf], np.float32)
    p3, _, _ = R.adam_ref_step(p, [None, bad], m, v, R.AdamRefState(), 1e-3, 0.9, 0.99, 1e-8, 0.0)
    assert np.isnan(p3[1]).all()                       # inf: m = inf, den = inf, inf / inf
    assert R.ulp_distance(np.float32([1.0, -1.0, 0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0])) == 1

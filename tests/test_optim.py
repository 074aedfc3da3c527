"""GPU tests of the optimiser stage (csrc/optim.hip, modules/optim.py): vpn_amd.Adam against the numpy
restatement tests/optim_ref.py, bit for bit, and against torch.optim.Adam through state dicts."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_ref as R

ULP_BOUND = R.ULP_BOUND

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.99), 1e-8          # the reference's betas (train.py:83)


def dev():
    return torch.device('cuda:0')


def chunk():
    from vpn_amd import ops
    return ops.ADAM_CHUNK


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
    return np.ascontiguousarray(a, dtype=np.float32).ravel().view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def gradient(rng, n):
    """magnitudes 1e-4 .. 1e1, either sign"""
    return (10.0 ** rng.uniform(-4, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def make_params(rng, sizes, misaligned=True):
    """Leaf tensors of the given sizes on the GPU, magnitudes 0.5 .. 2; with `misaligned`, one more that is a contiguous view
    4 bytes into a larger buffer."""
    d = dev()
    ps = [torch.from_numpy((rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)).to(d).requires_grad_(True)
          for n in sizes]
    if misaligned:
        n = chunk() + 9
        buf = torch.from_numpy(rng.uniform(0.5, 2.0, n + 1).astype(np.float32)).to(d)
        view = buf[1:]
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        ps.append(view.requires_grad_(True))
    return ps


class Ref:
    """The restatement's copy of one parameter group."""

    def __init__(self, params, lr, wd, betas=BETAS, eps=EPS):
        self.p = [p.detach().cpu().numpy().ravel().copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.state, self.lr, self.wd, self.betas, self.eps = R.AdamRefState(), lr, wd, betas, eps

    def step(self, grads, lr=None):
        grads = [None if g is None else np.asarray(g, dtype=np.float32).ravel() for g in grads]
        self.p, self.m, self.v = R.adam_ref_step(self.p, grads, self.m, self.v, self.state, self.lr if lr is None else lr,
                                                 self.betas[0], self.betas[1], self.eps, self.wd)

    def check(self, opt, params, what=''):
        for i, p in enumerate(params):
            st = opt.state[p]
            assert same_bits(p, self.p[i]), '%s: parameter %d' % (what, i)
            assert same_bits(st['exp_avg'], self.m[i]), '%s: exp_avg %d' % (what, i)
            assert same_bits(st['exp_avg_sq'], self.v[i]), '%s: exp_avg_sq %d' % (what, i)


def set_grads(params, grads):
    """Write `grads` (numpy, None = no gradient) into .grad, in place where a gradient tensor is already there."""
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif p.grad is None:
            p.grad = torch.from_numpy(g).to(p.device).view_as(p)
        else:
            p.grad.copy_(torch.from_numpy(g).view_as(p))


@pytest.mark.parametrize('zero_grad', [False, True])
@pytest.mark.parametrize('wd', [0.0, 1e-6])
def test_bit_exact_against_the_restatement(wd, zero_grad):
    import vpn_amd
    C = chunk()
    rng = np.random.default_rng(11)
    sizes = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7, 0, 6]                  # the last one never has a gradient
    params = make_params(rng, sizes)
    assert sum(p.numel() for p in params) < 200_000
    opt = vpn_amd.Adam(params, lr=1e-4, betas=BETAS, eps=EPS, weight_decay=wd)
    ref = Ref(params, 1e-4, wd)
    for it in range(4):
        grads = [gradient(rng, p.numel()) for p in params]
        grads[9] = None
        set_grads(params, grads)
        ptrs = [None if p.grad is None else p.grad.data_ptr() for p in params]
        assert params[10].grad.data_ptr() % 16 == 0                         # misaligned p, aligned g
        opt.step(zero_grad=zero_grad)
        ref.step(grads)
        ref.check(opt, params, 'step %d' % it)
        for p, g, ptr in zip(params, grads, ptrs):
            if g is None:
                assert p.grad is None
            else:
                assert p.grad.data_ptr() == ptr
                assert same_bits(p.grad, np.zeros_like(g) if zero_grad else g)
    assert opt.table_uploads == 1                                           # the pointers never changed
    assert opt.device_state()[0] == 4 and int(opt.state[params[0]]['step']) == 4


def test_two_groups_and_device_learning_rate():
    import vpn_amd
    rng = np.random.default_rng(12)
    many = make_params(rng, [1 + i % 7 for i in range(130)], misaligned=False)       # more than any by-value argument holds
    few = make_params(rng, [chunk() + 3, 17], misaligned=False)
    lr_dev = torch.tensor([1e-3], dtype=torch.float32, device=dev())
    opt = vpn_amd.Adam([{'params': many, 'lr': 5e-2, 'weight_decay': 0.0, 'lr_dev': lr_dev},
                        {'params': few, 'lr': 3e-4, 'weight_decay': 1e-6}], betas=BETAS, eps=EPS)
    assert 'lr_dev' not in opt.param_groups[0] and opt.param_groups[1]['lr'] == 3e-4
    ref_many, ref_few = Ref(many, None, 0.0), Ref(few, 3e-4, 1e-6)
    for it, lr in enumerate((1e-3, 2.5e-4, 7e-3)):
        lr_dev.fill_(lr)
        gm, gf = [gradient(rng, p.numel()) for p in many], [gradient(rng, p.numel()) for p in few]
        set_grads(many, gm)
        set_grads(few, gf)
        opt.step()
        ref_many.step(gm, lr=float(np.float32(lr)))                  # the kernel reads the float, not group['lr'] = 5e-2
        ref_few.step(gf)
        ref_many.check(opt, many, 'many, step %d' % it)
        ref_few.check(opt, few, 'few, step %d' % it)
    assert opt.table_uploads == 2 and opt.device_state(0)[0] == 3 and opt.device_state(1)[0] == 3
    # a scheduler writes group['lr']; the group without lr_dev follows it
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    gf = [gradient(rng, p.numel()) for p in few]
    set_grads(many, [None] * len(many))
    set_grads(few, gf)
    opt.step()
    sched.step()
    ref_few.step(gf)
    ref_few.check(opt, few, 'few, before the scheduler')
    ref_many.check(opt, many, 'many, no gradients')
    assert opt.device_state(0)[0] == 3 and opt.device_state(1)[0] == 4       # a group without gradients does not advance
    assert opt.param_groups[1]['lr'] == 1.5e-4
    set_grads(few, gf)
    opt.step()
    ref_few.step(gf, lr=1.5e-4)
    ref_few.check(opt, few, 'few, after the scheduler')


def test_step_and_state_advance():
    import vpn_amd
    from vpn_amd.modules.optim import advance_powers
    rng = np.random.default_rng(13)
    params = make_params(rng, [5, 3 * chunk() + 1], misaligned=False)       # one chunk and four: whichever arrives last
    opt = vpn_amd.Adam(params, lr=1e-4, betas=BETAS)
    assert opt.device_state() == (0, 1.0, 1.0, 0)
    set_grads(params, [gradient(rng, p.numel()) for p in params])
    for n in range(1, 8):
        opt.step()
        step, b1pow, b2pow, arrivals = opt.device_state()
        assert step == n and arrivals == 0
        assert (b1pow, b2pow) == advance_powers(n, *BETAS)                   # doubles: equal means bit-equal here
        assert (b1pow, b2pow) == (R.AdamRefState(n, *BETAS).b1pow, R.AdamRefState(n, *BETAS).b2pow)
    st = opt.state[params[1]]['step']
    assert st.is_cuda and st.dtype == torch.int64 and int(st) == 7 and st.data_ptr() == opt.state[params[0]]['step'].data_ptr()


def test_table_refresh():
    import vpn_amd
    rng = np.random.default_rng(14)
    params = make_params(rng, [7, chunk() + 1, 33, 12])
    opt = vpn_amd.Adam(params, lr=1e-4, betas=BETAS, weight_decay=1e-6)
    ref = Ref(params, 1e-4, 1e-6)

    def step(grads, what, uploads, fresh=False):
        if fresh:
            keep.extend(p.grad for p in params)          # the old tensors stay alive: the new ones have new addresses
            for p in params:
                p.grad = None
        set_grads(params, grads)
        opt.step()
        ref.step(grads)
        ref.check(opt, params, what)
        assert opt.table_uploads == uploads, what

    keep = []
    full = lambda: [gradient(rng, p.numel()) for p in params]
    g = full()
    g[3] = None
    step(g, 'first', 1)
    g = full()
    g[3] = None
    step(g, 'same pointers', 1)
    step(g, 'every gradient replaced', 2, fresh=True)
    g = full()
    g[3] = None
    g[0] = None
    step(g, 'one gradient gone', 3)
    g = full()
    g[0] = None
    step(g, 'a gradient for the parameter that had none', 4)
    step(g, 'same pointers again', 4)
    assert opt.device_state()[0] == 6


def _graph_case(seed):
    import vpn_amd
    rng = np.random.default_rng(seed)
    params = make_params(rng, [5, chunk() + 1, 2 * chunk()])
    opt = vpn_amd.Adam(params, lr=1e-4, betas=BETAS, weight_decay=1e-6)
    staging = [torch.zeros_like(p) for p in params]
    for p in params:
        p.grad = torch.zeros_like(p)

    def fill():
        grads = [gradient(rng, p.numel()) for p in params]
        for s, g in zip(staging, grads):
            s.copy_(torch.from_numpy(g).view_as(s))
        return grads

    def body():
        for p, s in zip(params, staging):
            p.grad.copy_(s)
        opt.step(zero_grad=True)

    return params, opt, Ref(params, 1e-4, 1e-6), fill, body


def test_no_sync_and_graph_capture():
    params, opt, ref, fill, body = _graph_case(15)
    ref.step(fill())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        body()                                   # the first step, table upload included, synchronises nowhere
    finally:
        torch.cuda.set_sync_debug_mode('default')
    ref.check(opt, params, 'eager')
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    assert opt.table_uploads == 1
    for it in range(3):
        ref.step(fill())
        graph.replay()
        ref.check(opt, params, 'replay %d' % it)
        assert all(not bool(p.grad.any()) for p in params)
    assert opt.device_state() == (4, ref.state.b1pow, ref.state.b2pow, 0)


def test_pointer_change_during_capture_raises():
    params, opt, ref, fill, body = _graph_case(16)
    fill()
    body()
    torch.cuda.synchronize()
    old = params[0].grad
    params[0].grad = torch.zeros_like(old)
    assert params[0].grad.data_ptr() != old.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='capture'):
        with torch.cuda.graph(graph):
            params[1].grad.mul_(1.0)                      # something to capture before the refusal
            opt.step()
    torch.cuda.synchronize()
    assert opt.table_uploads == 1 and opt.device_state()[0] == 1
    opt.step()                                            # outside a capture the same change is an upload
    assert opt.table_uploads == 2 and opt.device_state()[0] == 2


def test_deterministic():
    import vpn_amd
    outs = []
    for _ in range(2):
        rng = np.random.default_rng(17)
        params = make_params(rng, [3, 4 * chunk() + 5, chunk()])
        opt = vpn_amd.Adam(params, lr=1e-3, betas=BETAS, weight_decay=1e-6)
        for _ in range(3):
            set_grads(params, [gradient(rng, p.numel()) for p in params])
            opt.step()
        outs.append([bits(t) for p in params for t in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'])])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_state_dict_interop():
    import vpn_amd
    rng = np.random.default_rng(18)
    sizes = [9, chunk() + 2, 130]
    params = make_params(rng, sizes, misaligned=False)
    start = [p.detach().clone() for p in params]
    grads = [[gradient(rng, p.numel()) for p in params] for _ in range(5)]
    hyper = dict(lr=1e-4, betas=BETAS, eps=EPS, weight_decay=1e-6)
    opt = vpn_amd.Adam(params, **hyper)
    for g in grads[:3]:
        set_grads(params, g)
        opt.step()
    sd = opt.state_dict()
    assert sorted(sd['param_groups'][0]) == sorted(torch.optim.Adam([nn.Parameter(torch.zeros(1))]).state_dict()['param_groups'][0])
    assert sorted(sd['state'][1]) == ['exp_avg', 'exp_avg_sq', 'step']
    assert float(sd['state'][1]['step']) == 3.0 and sd['state'][1]['step'].device.type == 'cpu'
    at3 = [p.detach().clone() for p in params]
    for g in grads[3:]:
        set_grads(params, g)
        opt.step()

    # resumed: a fresh optimiser over clones of the parameters as they were at step 3
    resumed = [p.clone().requires_grad_(True) for p in at3]
    opt2 = vpn_amd.Adam(resumed, lr=1.0, betas=(0.5, 0.5))               # every hyper-parameter comes from the state dict
    opt2.load_state_dict(sd)
    assert opt2.device_state() == (3,) + vpn_amd.modules.optim.advance_powers(3, *BETAS) + (0,)
    for g in grads[3:]:
        set_grads(resumed, g)
        opt2.step()
    for a, b in zip(params, resumed):
        assert same_bits(a, b)
        assert same_bits(opt.state[a]['exp_avg'], opt2.state[b]['exp_avg'])
        assert same_bits(opt.state[a]['exp_avg_sq'], opt2.state[b]['exp_avg_sq'])
    assert int(opt2.state[resumed[0]]['step']) == 5

    # the same dict in torch.optim.Adam: its next step stays within the bound measured against torch on the CPU
    ref = Ref(at3, 1e-4, 1e-6)
    ref.m = [sd['state'][i]['exp_avg'].cpu().numpy().ravel().copy() for i in range(3)]
    ref.v = [sd['state'][i]['exp_avg_sq'].cpu().numpy().ravel().copy() for i in range(3)]
    ref.state = R.AdamRefState(3, *BETAS)
    ref.step(grads[3])
    theirs = [p.clone().requires_grad_(True) for p in at3]
    topt = torch.optim.Adam(theirs, lr=1.0)
    topt.load_state_dict(sd)                     # torch adopts the dict's tensors: its step below updates them in place
    set_grads(theirs, grads[3])
    topt.step()
    for i, t in enumerate(theirs):
        d = R.ulp_distance(t.detach().cpu().numpy(), ref.p[i])
        print('torch.optim.Adam after our state dict, parameter %d: %d ulp' % (i, d))
        assert d <= ULP_BOUND
        assert float(topt.state[t]['step']) == 4.0

    # and a torch.optim.Adam state dict loads here: three torch steps, then two of ours against the restatement
    theirs = [p.clone().requires_grad_(True) for p in start]
    topt = torch.optim.Adam(theirs, **hyper)
    for g in grads[:3]:
        set_grads(theirs, g)
        topt.step()
    ours = [p.detach().clone().requires_grad_(True) for p in theirs]
    opt3 = vpn_amd.Adam(ours, lr=1.0)
    opt3.load_state_dict(topt.state_dict())
    assert opt3.device_state()[0] == 3 and opt3.param_groups[0]['lr'] == 1e-4 and opt3.param_groups[0]['betas'] == BETAS
    ref = Ref(ours, 1e-4, 1e-6)
    ref.m = [topt.state[t]['exp_avg'].cpu().numpy().ravel().copy() for t in theirs]
    ref.v = [topt.state[t]['exp_avg_sq'].cpu().numpy().ravel().copy() for t in theirs]
    ref.state = R.AdamRefState(3, *BETAS)
    for g in grads[3:]:
        set_grads(ours, g)
        opt3.step()
        ref.step(g)
    ref.check(opt3, ours, 'after a torch state dict')


class Mix(nn.Module):
    """A 1x1 channel mix by matmul (no convolution library is involved)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin) / cin ** 0.5)

    def forward(self, x):
        return torch.einsum('oc,bchw->bohw', self.weight, x)


class PlainTrunk(nn.Module):
    def __init__(self, feat=40):
        super().__init__()
        self.conv1, self.bn1, self.relu, self.maxpool = Mix(3, 8), nn.Identity(), nn.ReLU(), nn.AvgPool2d(2)
        self.layer1, self.layer2, self.layer3, self.layer4 = Mix(8, 8), Mix(8, 16), Mix(16, 16), Mix(16, feat)


def test_whole_model():
    """One forward and backward of VPNetOneRes through the existing path (ATen trunk, FC heads on csrc/fcstack.hip), then
    one step: every parameter equals the restatement applied to the same gradients, and the heads' gradients, which
    fc_bwd_kernel wrote, are consumed (and zeroed) where they lie."""
    import vpn_amd
    d = dev()
    torch.manual_seed(5)
    K = 2
    net = vpn_amd.VPNetOneRes(vp_num=K, hidden=72, feat=40, trunk=PlainTrunk()).to(d)
    imgs = torch.rand(2, 3, 16, 16, device=d)
    u = torch.rand(2, K, 32, 3, device=d)
    params = list(net.parameters())
    opt = vpn_amd.Adam(params, lr=1e-3, betas=BETAS, weight_decay=1e-6)
    ref = Ref(params, 1e-3, 1e-6)
    before = [p.detach().clone() for p in params]
    packed, _, _ = net.forward_packed(imgs)
    vpn_amd.Sampling.sample_primitives(packed, [1, 0], 32, u=u).square().sum().backward()
    assert all(p.grad is not None for p in params)
    heads = [t for head in net.head_linears() for m in head for t in (m.weight, m.bias)]
    assert len(heads) == 30 and all(bool(t.grad.any()) for t in heads)
    grads = [p.grad.detach().cpu().numpy().copy() for p in params]
    ptrs = [p.grad.data_ptr() for p in params]
    opt.step(zero_grad=True)
    ref.step(grads)
    ref.check(opt, params, 'whole model')
    assert all(not same_bits(p, b) for p, b in zip(params, before))          # every parameter moved
    assert all(p.grad.data_ptr() == ptr and not bool(p.grad.any()) for p, ptr in zip(params, ptrs))
    assert opt.table_uploads == 1 and opt.device_state()[0] == 1

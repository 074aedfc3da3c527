"""The optimiser stage (csrc/optim.hip): `Adam(params, lr, betas=(0.9, 0.99), weight_decay=W_DECAY)` and
`optimizer.step()` of the reference (train.py:83-102, :264; train_sphere.py:92, :134; train_gcn.py:105, :138) as ONE launch per
parameter group, with the step counter and the bias-correction products on the device and, on request, the gradient zeroing
of train.py:262 in the same pass.  GPU only: there is no eager fall-back."""
import struct

import torch

from .. import _lib, ops

_ALIGN = 4                               # every parameter's slice of the flat m / v buffers starts on 16 bytes


def _torch_adam_defaults():
    """torch.optim.Adam's own `defaults` (the keys of a param group differ between torch versions): a state dict made here
    carries exactly the keys the installed torch.optim.Adam expects, and the other way round."""
    return dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)


def advance_powers(steps, beta1, beta2):
    """(beta1 ** steps, beta2 ** steps) as the kernel forms them: one double multiplication per step, starting from 1.0."""
    b1pow = b2pow = 1.0
    for _ in range(int(steps)):
        b1pow *= beta1
        b2pow *= beta2
    return b1pow, b2pow


class _Group:
    """What a parameter group owns on the device: the flat m and v buffers, the state block {int64 step, double b1pow,
    double b2pow, uint32 arrivals} and the tables of the last upload."""

    def __init__(self, params, lr_dev):
        self.device = params[0].device
        offsets, total = [], 0
        for p in params:
            offsets.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.exp_avg = torch.zeros(max(total, _ALIGN), dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.views = {p: (self.exp_avg[o:o + p.numel()].view_as(p), self.exp_avg_sq[o:o + p.numel()].view_as(p))
                      for p, o in zip(params, offsets)}
        self.pointers = {p: (m.data_ptr(), v.data_ptr()) for p, (m, v) in self.views.items()}
        self.block = torch.empty(_lib.CONSTANTS['VPN_ADAM_STATE_BYTES'] // 8, dtype=torch.int64, device=self.device)
        self.step = self.block[0]                                   # a view of the block: the device step
        self.set_step(0, 1.0, 1.0)
        self.lr_dev = lr_dev
        self.key = None                      # (p pointer, g pointer, size) per row of the last upload
        self.segments = self.chunks = None   # device tables (two views of one buffer)
        self.num_segments = self.num_chunks = 0

    def set_step(self, step, b1pow, b2pow):
        bits = struct.unpack('<4q', struct.pack('<qddII', int(step), b1pow, b2pow, 0, 0))
        self.block.copy_(torch.tensor(bits, dtype=torch.int64))


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's algorithm (L2 weight decay, no amsgrad) on csrc/optim.hip: one launch per parameter group whatever
    the number of parameters, no host synchronisation, and nothing per step on the host but a comparison of pointers.

    Param groups, zero_grad, LR schedulers (they write group['lr'], read at every step) and add_param_group work as in torch.
    `lr_dev` (the keyword, or the key 'lr_dev' of a param group dict): a one-element fp32 tensor on the device that the
    kernel reads INSTEAD of group['lr'], so that a captured graph follows a schedule written on the device.
    `step(zero_grad=True)` also writes 0 to every gradient it consumed, in the same pass (the gradients stay allocated).

    State: per group one flat buffer for m and one for v; state[p]['exp_avg'] / ['exp_avg_sq'] are views into them and
    state[p]['step'] is a view of the group's device step counter (int64).  state_dict() / load_state_dict() use
    torch.optim.Adam's layout, so a state dict moves both ways between the two optimisers; after a load the bias-correction
    products are recomputed by the same repeated double multiplication, so a resumed run equals an uninterrupted one bit
    for bit.

    ONE deliberate difference from torch: the step count is per GROUP, not per parameter.  A parameter that had no gradient
    for some steps keeps its m and v meanwhile and, when it has one again, uses the group's bias correction (torch would
    use the parameter's own, smaller, count).  Loading a torch state dict whose parameters of one group have different
    counts takes the largest.

    The arithmetic is the one include/vpn_hip.h states for vpn_adam_step; tests/optim_ref.py restates it bit for bit.  It
    differs from torch's kernels in the last bits (they contract and order some operations differently)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, lr_dev=None, amsgrad=False,
                 maximize=False):
        if amsgrad:
            raise ValueError('vpn_amd.Adam: amsgrad is not implemented (there is no fall-back to torch.optim.Adam)')
        if maximize:
            raise ValueError('vpn_amd.Adam: maximize is not implemented (there is no fall-back to torch.optim.Adam)')
        if isinstance(lr, torch.Tensor):
            raise ValueError('vpn_amd.Adam: lr is a number; a learning rate on the device goes to lr_dev')
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid betas: %r' % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        defaults = _torch_adam_defaults()
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._groups = []                    # _Group of param_groups[i]
        self._default_lr_dev = lr_dev
        self.table_uploads = 0               # how often step() had to upload a table (tests: unchanged pointers upload none)
        super().__init__(params, defaults)

    # ---- construction

    def add_param_group(self, param_group):
        lr_dev = param_group.pop('lr_dev', self._default_lr_dev) if isinstance(param_group, dict) else self._default_lr_dev
        before = len(self.param_groups)
        super().add_param_group(param_group)
        group = self.param_groups[before]
        if group.get('amsgrad') or group.get('maximize'):
            del self.param_groups[before]
            raise ValueError('vpn_amd.Adam: amsgrad / maximize are not implemented')
        try:
            params = group['params']
            if not params:
                raise ValueError('vpn_amd.Adam: a parameter group needs at least one parameter')
            for p in params:
                if p.dtype != torch.float32:
                    raise ValueError('vpn_amd.Adam: parameters must be fp32, got %s' % p.dtype)
                if not p.is_contiguous():
                    raise ValueError('vpn_amd.Adam: parameters must be contiguous')
                if not p.is_cuda:
                    raise RuntimeError('vpn_amd.Adam runs on the GPU only (got a %s parameter); there is no CPU path' % p.device.type)
                if p.device != params[0].device:
                    raise ValueError('vpn_amd.Adam: the parameters of one group must be on one device')
            if lr_dev is not None and not (isinstance(lr_dev, torch.Tensor) and lr_dev.dtype == torch.float32 and
                                           lr_dev.numel() == 1 and lr_dev.device == params[0].device):
                raise ValueError('vpn_amd.Adam: lr_dev must be a one-element fp32 tensor on the parameters\' device')
            g = _Group(params, lr_dev)
        except Exception:
            del self.param_groups[before]
            raise
        self._groups.append(g)
        for p in params:
            self.state[p] = {'step': g.step, 'exp_avg': g.views[p][0], 'exp_avg_sq': g.views[p][1]}

    # ---- the step

    def _refresh(self, group, g):
        """Make g's device tables describe the parameters of `group` that have a gradient now; upload only on a change."""
        entries, key = [], []
        for p in group['params']:
            grad = p.grad
            if grad is None:
                continue
            if grad.is_sparse or grad.dtype != torch.float32 or grad.device != p.device or not grad.is_contiguous():
                raise RuntimeError('vpn_amd.Adam: gradients must be dense contiguous fp32 tensors on the parameter\'s device')
            entries.append((p.data_ptr(), grad.data_ptr()) + g.pointers[p] + (p.numel(),))
            key.append((entries[-1][0], entries[-1][1], entries[-1][4]))
        if key == g.key:
            return
        if entries and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('vpn_amd.Adam: the set of (parameter, gradient) tensors changed during stream capture; run '
                               'one step with the same tensors before capturing, and keep every .grad allocated')
        segments, chunks = ops.adam_tables(entries)
        g.num_segments, g.num_chunks = len(segments), len(chunks)
        if segments:
            words = [w for row in segments for w in row] + [w for row in chunks for w in row]
            # new buffers on both sides: a launch or a copy that is still queued keeps the old ones, and both allocators
            # hand them out again only behind that work
            host = torch.tensor(words, dtype=torch.int64).pin_memory()
            table = torch.empty(len(words), dtype=torch.int64, device=g.device)
            table.copy_(host, non_blocking=True)             # the one copy
            g.segments, g.chunks = table[:6 * len(segments)], table[6 * len(segments):]
            self.table_uploads += 1
        g.key = key

    @torch.no_grad()
    def step(self, closure=None, *, zero_grad=False):
        """One Adam step of every group that has gradients: one launch per group on the current stream, no host
        synchronisation.  zero_grad: the gradients are zero afterwards (written by the same launch, still allocated).
        A group none of whose parameters has a gradient launches nothing and does not advance its step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group, g in zip(self.param_groups, self._groups):
            self._refresh(group, g)
            if g.num_segments == 0 or g.num_chunks == 0:
                continue
            ops.adam_step(g.segments, g.num_segments, g.chunks, g.num_chunks, g.block, float(group['lr']), g.lr_dev,
                          float(group['betas'][0]), float(group['betas'][1]), float(group['eps']), float(group['weight_decay']),
                          zero_grad)
        return loss

    # ---- state dicts in torch.optim.Adam's layout

    def state_dict(self):
        """torch.optim.Adam's layout: per parameter `step` (a CPU fp32 scalar, the group's count), `exp_avg`, `exp_avg_sq`;
        the param_groups keys of the installed torch.  A snapshot: the moments are copies, not the live views (which the
        next step would change under a count that was read now).  Reads the device steps (synchronises)."""
        sd = super().state_dict()
        steps = {}
        for g, group in zip(self._groups, sd['param_groups']):
            count = int(g.step.item())
            for i in group['params']:
                steps[i] = count
        for i, st in sd['state'].items():
            sd['state'][i] = {'step': torch.tensor(float(steps[i]), dtype=torch.float32), 'exp_avg': st['exp_avg'].clone(),
                              'exp_avg_sq': st['exp_avg_sq'].clone()}
        return sd

    def load_state_dict(self, state_dict):
        """Takes a state dict of this class or of torch.optim.Adam.  The loaded moments are copied into the groups' flat
        buffers; the group's step is the (largest) loaded count and b1pow / b2pow are recomputed from it on the host by
        the kernel's own repeated multiplication."""
        for group in state_dict['param_groups']:
            if group.get('amsgrad') or group.get('maximize') or group.get('decoupled_weight_decay'):
                raise ValueError('vpn_amd.Adam: cannot load a state made with amsgrad, maximize or decoupled weight decay')
        super().load_state_dict(state_dict)
        loaded = self.state
        state = type(loaded)(dict)
        for group, g in zip(self.param_groups, self._groups):
            count = 0
            for p in group['params']:
                m, v = g.views[p]
                st = loaded.get(p)
                if st:
                    m.copy_(st['exp_avg'].reshape(m.shape))
                    v.copy_(st['exp_avg_sq'].reshape(v.shape))
                    count = max(count, int(round(float(st['step']))))
                else:
                    m.zero_()
                    v.zero_()
                state[p] = {'step': g.step, 'exp_avg': m, 'exp_avg_sq': v}
            g.set_step(count, *advance_powers(count, float(group['betas'][0]), float(group['betas'][1])))
        self.state = state

    def device_state(self, index=0):
        """(step, b1pow, b2pow, arrivals) of group `index`, read from the device (synchronises; for tests and logs)."""
        raw = self._groups[index].block.cpu().numpy().tobytes()
        return struct.unpack('<qddII', raw)[:4]

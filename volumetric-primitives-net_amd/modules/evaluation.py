"""The evaluation loops of the reference (test.py:68-135, test_gcn.py:115-178) on csrc/evaluate.hip: per-sample Chamfer
and EMD metrics of every batch and the per-class bookkeeping of the epoch, kept on the device.

    meter = EvaluationMeter(class_names, device)               # emd=False: Chamfer only, the test.py form
    for data in dataloader:
        ...
        meter.update(predict_points, gt_points, data['class_index'])
    meter.report(epoch)

`update` makes no host synchronisation (the reference makes 2 + 2 B per batch through .item()) and can be captured into a
HIP graph; `result` is the ONE device-to-host copy of an epoch.

The total is what the reference computes: the mean over batches of the batch means (test.py:104,126, test_gcn.py:145-146,
163-164), so a short last batch weighs like a full one.  Unlike test.py:105, which walks range(BATCH_SIZE), the class loop
runs over the batch's real size: a short last batch does not crash.

The one deliberate deviation: a class index outside [0, len(class_names)) makes the reference raise IndexError (or, when
negative, silently count the sample for a class from the end).  Raising needs a synchronisation; here the sample is left out
of every class sum, still enters the batch mean like in the reference, and `result()['n_invalid']` counts it.

The visual dumps of the evaluation scripts (Visualizer.render_*, test.py:110-124) are modules/visualize.py."""
import torch

from .. import dist as vdist
from .. import ops


class EvaluationMeter:
    def __init__(self, class_names, device, emd=True, eps=0.005, iters=50, cd_scale=1.0):
        """class_names: the caller's list (the reference's 13 ShapeNet names are its data; there is no default).
        emd=True: Chamfer and EMD on equally large clouds (test_gcn.py:142-143, auction with eps, iters as :81);
        emd=False: Chamfer only.  cd_scale multiplies every per-sample Chamfer value (test.py:101: L_VIEW_CD).
        A meter on the CPU holds a state for result() / report() / merge(); update() needs the GPU."""
        self.class_names = [str(c) for c in class_names]
        if not self.class_names:
            raise ValueError('EvaluationMeter needs at least one class name')
        self.C = len(self.class_names)
        self.device = torch.device(device)
        self.emd, self.eps, self.iters, self.cd_scale = bool(emd), float(eps), int(iters), float(cd_scale)
        self.state = ops.eval_state(self.C, self.device)

    def _class_index(self, class_indices, B):
        if isinstance(class_indices, torch.Tensor) and class_indices.is_cuda:
            idx = class_indices.reshape(-1).to(torch.int32)
        else:
            # what the reference's DataLoader yields (a CPU int64 tensor) or a list: up through pinned memory, no blocking
            idx = torch.as_tensor(class_indices).reshape(-1).to(torch.int32).pin_memory().to(self.device, non_blocking=True)
        if idx.numel() != B:
            raise ValueError('%d class indices for a batch of %d' % (idx.numel(), B))
        return idx

    @torch.no_grad()
    def update(self, predict_points, gt_points, class_indices, max_group=None):
        """One batch: predict_points [B,N,3], gt_points [B,M,3] on the device (N == M when emd), class_indices [B] (a device
        tensor, a CPU tensor or a list).  Returns the per-sample metrics (cd_b [B], emd_b [B] or None) as device tensors."""
        assert predict_points.ndimension() == 3 and gt_points.ndimension() == 3        # (B, N, 3)  chamfer_distance.py:32-35
        B, N, M = predict_points.size(0), predict_points.size(1), gt_points.size(1)
        if self.emd and N != M:            # before any launch or upload
            raise ValueError('the EMD metric needs as many predicted as ground-truth points (emd_module.py:36): %d vs %d'
                             % (N, M))
        if not (predict_points.is_cuda and gt_points.is_cuda):
            raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path'
                               % predict_points.device.type)
        return ops.eval_step(predict_points, gt_points, self._class_index(class_indices, B), self.state, self.C, emd=self.emd,
                             eps=self.eps, iters=self.iters, cd_scale=self.cd_scale, max_group=max_group)

    def reset(self):
        self.state.zero_()

    def load_state(self, state):
        """Replace the meter's state by a copy of `state` (a state tensor of the same number of classes, any device)."""
        ops.eval_state_fields(state, self.C)
        self.state.copy_(state)

    @staticmethod
    def merge(state_a, state_b):
        """The state of two evaluations taken together: the field-wise sum of two state tensors (sums as float64, counts
        as int64).  What result(group=...) does across ranks, without a process group; works on CPU tensors."""
        if state_a.shape != state_b.shape or (state_a.numel() - 5) % 3:
            raise ValueError('merge needs two evaluation states of the same number of classes')
        C = (state_a.numel() - 5) // 3
        out = torch.empty_like(state_a)
        (sa, na), (sb, nb), (so, no) = (ops.eval_state_fields(t, C) for t in (state_a, state_b.to(state_a.device), out))
        torch.add(sa, sb, out=so)
        torch.add(na, nb, out=no)
        return out

    def result(self, group=None):
        """The epoch so far as plain Python: {'cd': total_cd / n_batches, 'emd': ... (None without EMD), 'class_cd': [...],
        'class_emd': [...], 'class_n': [...], 'n_batches', 'n_invalid'}; a class that never occurred gives None.
        group: a torch.distributed process group whose ranks each evaluated a shard: their states are summed by one
        all-reduce first, so every rank reports the whole set.  One device-to-host copy."""
        state = self.state if group is None else vdist.all_reduce_eval_state(self.state, self.C, group)
        sums, counts = ops.eval_state_fields(state.cpu(), self.C)
        sums, counts = sums.tolist(), counts.tolist()
        C = self.C
        n_batches, n_invalid, class_n = counts[0], counts[1], counts[2:]
        per_class = lambda s: [s[c] / class_n[c] if class_n[c] else None for c in range(C)]
        return {'cd': sums[0] / n_batches if n_batches else None,
                'emd': (sums[1] / n_batches if n_batches else None) if self.emd else None,
                'class_cd': per_class(sums[3:3 + C]),
                'class_emd': per_class(sums[3 + C:3 + 2 * C]) if self.emd else [None] * C,
                'class_n': class_n, 'n_batches': n_batches, 'n_invalid': n_invalid}

    def report(self, epoch=None, group=None):
        """Prints what test_gcn.py:165-178 prints (Chamfer only: test.py:127-135): one line per class that occurred, then
        the total; a line for n_invalid when it is not zero.  Returns result()."""
        res = self.result(group)
        head = '\nEpoch %d\n' % epoch if epoch is not None else ''
        fmt = lambda v: float('nan') if v is None else v
        if self.emd:
            print(head)
            print('=' * 30)
            for i, name in enumerate(self.class_names):
                if res['class_n'][i] == 0:
                    continue
                print(name, '\t\tcd loss = %.6f, emd loss = %.6f' % (res['class_cd'][i], res['class_emd'][i]))
            print('=' * 30)
            print('total \t\tcd loss = %.6f, emd loss = %.6f' % (fmt(res['cd']), fmt(res['emd'])))
        else:
            print(head + '============================')
            for i, name in enumerate(self.class_names):
                if res['class_n'][i] == 0:
                    continue
                print(name, 'avg cd loss = %.6f' % res['class_cd'][i])
            print('============================\ntotal avg cd loss = %.6f' % fmt(res['cd']))
        if res['n_invalid']:
            print('n_invalid = %d (class index outside [0, %d): in the total, in no class)' % (res['n_invalid'], self.C))
        return res

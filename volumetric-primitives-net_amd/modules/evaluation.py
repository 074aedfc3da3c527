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

The visual dumps of the evaluation scripts (Visualizer.render_*, test.py:110-124) are modules/visualize.py.

SurfaceEvaluationMeter (csrc/surfeval.hip) is the same kind of meter for the metrics the reference does not
report: Chamfer-L2 / -L1, precision / recall / F-score at distance thresholds and normal consistency on points sampled from
the predicted SURFACE, which, unlike the vertices, see a triangle that cuts through empty space.

VolumeEvaluationMeter (csrc/occupancy.hip) is the meter for volumetric IoU: the prediction -- a primitive
assembly with its closed-form inside test, or a triangle mesh through its generalized winding number -- and the ground-truth
mesh are asked "is x inside" on one grid of query points, and the occupied sets are compared per sample."""
import math

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


class SurfaceEvaluationMeter:
    """Per-class surface metrics of an evaluation epoch, kept on the device (csrc/surfeval.hip):

        meter = SurfaceEvaluationMeter(class_names, device, thresholds=(0.01, 0.02))
        for data in dataloader:
            ...
            meter.update_mesh(predict_vertices, faces, gt_points, data['class_index'], seed=step)
        meter.report(epoch)

    Like EvaluationMeter, `update` makes no host synchronisation, can be captured into a HIP graph and is bit-equal from run
    to run; `result` is the ONE device-to-host copy of an epoch.  Unlike it, the totals are SAMPLE-weighted: the sum over
    all samples divided by n_samples.  EvaluationMeter's mean over batch means is the reference's rule for the reference's
    two metrics; these metrics have no reference to imitate, so they take the standard definition, under which a short last
    batch weighs by its samples.  A class index outside [0, C) enters the totals, no class, and n_invalid.

    Per sample, with nearest-neighbour distances d1 (prediction -> ground truth) and d2 (the other way) as chamfer_nn gives
    them (Euclidean, not squared; squares are formed in fp64, where they are exact):
        accuracy = mean d1^2, completeness = mean d2^2, cd = accuracy + completeness               (Chamfer-L2)
        cd_l1 = (mean d1 + mean d2) / 2                                                             (Chamfer-L1)
        precision_t = #{d1^2 < tau_t^2} / N, recall_t = #{d2^2 < tau_t^2} / M, fscore_t = 2 P R / (P + R), 0 when P + R = 0
        normal_consistency = (mean |n_pred . n_gt[nearest]| + mean |n_gt . n_pred[nearest]|) / 2
    and an epoch figure is the mean of the per-sample figure (cd and cd_l1 of the means of their two halves)."""

    def __init__(self, class_names, device, thresholds=(0.01, 0.02)):
        """thresholds: DISTANCES (not squared); the default is 1 % and 2 % of the unit box the data lives in.  The kernel
        compares squared distances with float32(tau * tau), the product formed in float64, uploaded once here."""
        self.class_names = [str(c) for c in class_names]
        if not self.class_names:
            raise ValueError('SurfaceEvaluationMeter needs at least one class name')
        self.C = len(self.class_names)
        self.device = torch.device(device)
        self.thresholds = [float(t) for t in thresholds]
        self.T = len(self.thresholds)
        ops.surfeval_width(self.T)
        if not all(math.isfinite(t) and t > 0.0 for t in self.thresholds):
            raise ValueError('thresholds must be positive finite distances, got %r' % (self.thresholds,))
        self.W = 6 + 3 * self.T
        thr2 = torch.tensor([t * t for t in self.thresholds], dtype=torch.float64).to(torch.float32)
        self.thr2 = thr2.pin_memory().to(self.device, non_blocking=True) if self.device.type == 'cuda' else thr2
        self.state = ops.surfeval_state(self.C, self.T, self.device)
        self.has_normals = False            # a host flag: whether any batch of the epoch carried normals (no read-back)

    _class_index = EvaluationMeter._class_index

    @torch.no_grad()
    def update(self, predict_points, gt_points, class_indices, predict_normals=None, gt_normals=None):
        """One batch: predict_points [B,N,3], gt_points [B,M,3] on the device (N and M may differ), class_indices [B] (a
        device tensor, a CPU tensor or a list), unit normals [B,N,3] / [B,M,3] for both or for neither.  Returns the
        per-sample rows [B, 6 + 3 T] (include/vpn_hip.h lists the columns) as a device tensor."""
        if not (isinstance(predict_points, torch.Tensor) and isinstance(gt_points, torch.Tensor)
                and predict_points.dim() == 3 and gt_points.dim() == 3):
            raise ValueError('predict_points [B,N,3] and gt_points [B,M,3] expected')
        if (predict_normals is None) != (gt_normals is None):
            raise ValueError('normals of the prediction and of the ground truth come together or not at all')
        if not (predict_points.is_cuda and gt_points.is_cuda):
            raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path'
                               % predict_points.device.type)
        rows = ops.surfeval_step(predict_points, gt_points, self._class_index(class_indices, predict_points.size(0)), self.state,
                                 self.C, self.thr2, predict_normals, gt_normals)
        self.has_normals = self.has_normals or predict_normals is not None
        return rows

    @torch.no_grad()
    def update_mesh(self, verts, faces, gt_points, class_indices, *, n=2048, seed, mesh_base=0, gt_normals=None):
        """One batch of predicted MESHES: verts [B,P,3], one faces [F,3] for the batch (int32 or int64, host or device).
        ops.sample_meshes draws n area-weighted surface points per mesh (Philox(seed; mesh_base + b, point)); with
        gt_normals [B,M,3] the normals of their faces are taken (ops.face_normals_at) and normal consistency is measured,
        without them that step is skipped; then `update`.  Returns the per-sample rows."""
        if not (isinstance(verts, torch.Tensor) and verts.dim() == 3 and verts.size(-1) == 3):
            raise ValueError('verts [B,P,3] expected')
        if not verts.is_cuda:
            raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % verts.device.type)
        verts = verts.detach()
        f32 = ops.faces_i32(faces, verts.device)
        points, fidx, _ = ops.sample_meshes(verts, f32, n, seed, mesh_base)
        normals = None if gt_normals is None else ops.face_normals_at(verts.float().contiguous(), f32, fidx)
        return self.update(points, gt_points, class_indices, normals, gt_normals)

    @torch.no_grad()
    def update_surface(self, surface, gt_points, class_indices, *, n=2048, seed, mesh_base=0, gt_normals=None):
        """One batch of EXTRACTED surfaces (ops.IsoSurface): one closed mesh per sample whose size the host
        does not know.  ops.ragged_sample draws n area-weighted points per mesh on the padded layout (Philox(seed; mesh_base
        + b, point), as update_mesh; a padding face has no area and is never drawn); with gt_normals [B,M,3] the normals of
        their faces are taken (ops.ragged_face_normals); a sample whose counts say no faces or overflow gets class index -1
        on the device, so it lands in n_invalid and in no class; then `update`.  No host synchronisation.  Returns the
        per-sample rows."""
        if not (hasattr(surface, 'arrays') and hasattr(surface, 'counts')):
            raise TypeError('surface must be an ops.IsoSurface (ops.isosurface / Meshing.union_meshes)')
        if not surface.verts.is_cuda:
            raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % surface.verts.device.type)
        B = len(surface)
        arrays = surface.arrays()
        points, fidx, _ = ops.ragged_sample(*arrays, n, seed=seed, mesh_base=mesh_base, return_faces=True)
        normals = None
        if gt_normals is not None:
            normals = ops.ragged_face_normals(arrays.verts, arrays.faces, arrays.vert_offset, arrays.face_offset, fidx)[:, 0].contiguous()
        idx = self._class_index(class_indices, B)
        unusable = (surface.counts[:, 1] == 0) | (surface.counts[:, 3] != 0)
        return self.update(points[:, 0].contiguous(), gt_points, torch.where(unusable, torch.full_like(idx, -1), idx), normals,
                           gt_normals)

    @torch.no_grad()
    def update_primitives(self, params, kinds, gt_points, class_indices, *, resolution=64, bounds=(-0.5, 0.5), n=2048, seed,
                          mesh_base=0, gt_normals=None, level=0.0, **capacity):
        """One batch of predicted primitive assemblies, scored on their OUTER surface: Meshing.union_meshes(params, kinds,
        resolution, bounds, level, **capacity), then update_surface.  Points sampled from the primitives one by one
        (Sampling.sample_primitives) also lie on the walls inside another primitive; these do not."""
        from .meshing import Meshing
        surface = Meshing.union_meshes(params, kinds, resolution=resolution, bounds=bounds, level=level, **capacity)
        return self.update_surface(surface, gt_points, class_indices, n=n, seed=seed, mesh_base=mesh_base, gt_normals=gt_normals)

    def reset(self):
        self.state.zero_()
        self.has_normals = False

    def load_state(self, state, has_normals=True):
        """Replace the meter's state by a copy of `state` (a state tensor of the same classes and thresholds, any device).
        has_normals: whether the loaded epoch measured normal consistency (a state does not say)."""
        ops.surfeval_state_fields(state, self.C, self.T)
        self.state.copy_(state)
        self.has_normals = bool(has_normals)

    @staticmethod
    def merge(state_a, state_b, T=2):
        """The state of two evaluations taken together: the field-wise sum of two state tensors of the same classes and
        thresholds (sums as float64, counts as int64).  What result(group=...) does across ranks, without a process group;
        works on CPU tensors.  T: the number of thresholds of both (the default meter has 2); the number of classes follows
        from the size."""
        W = ops.surfeval_width(T)
        if state_a.shape != state_b.shape or state_a.dim() != 1 or state_a.numel() < 2 * W + 4 or (state_a.numel() - 3 - W) % (W + 1):
            raise ValueError('merge needs two surface evaluation states of the same number of classes and of %d thresholds' % T)
        C = (state_a.numel() - 3 - W) // (W + 1)
        out = torch.empty_like(state_a)
        (sa, na), (sb, nb), (so, no) = (ops.surfeval_state_fields(t, C, T) for t in (state_a, state_b.to(state_a.device), out))
        torch.add(sa, sb, out=so)
        torch.add(na, nb, out=no)
        return out

    def result(self, group=None):
        """The epoch so far as plain Python.  Epoch figures: 'cd' (accuracy + completeness), 'cd_l1', 'accuracy',
        'completeness', 'normal_consistency' (None when no batch of the epoch carried normals), 'precision', 'recall',
        'fscore' (lists of T); per class the same keys as 'class_*' lists, None for a class that never occurred; 'class_n',
        'n_samples', 'n_batches', 'n_invalid', 'thresholds'.  group: a torch.distributed process group whose ranks each
        evaluated a shard: their states are summed by one all-reduce first.  One device-to-host copy."""
        state = self.state if group is None else vdist.all_reduce_surfeval_state(self.state, self.C, self.T, group)
        sums, counts = ops.surfeval_state_fields(state.cpu(), self.C, self.T)
        sums, counts = sums.tolist(), counts.tolist()
        C, T, W = self.C, self.T, self.W
        n_samples, n_batches, n_invalid, class_n = counts[0], counts[1], counts[2], counts[3:]

        def figures(row, n):
            if not n:
                return None
            m = [v / n for v in row]
            return {'cd': m[0] + m[1], 'cd_l1': 0.5 * (m[2] + m[3]), 'accuracy': m[0], 'completeness': m[1],
                    'normal_consistency': 0.5 * (m[4] + m[5]) if self.has_normals else None,
                    'precision': m[6:6 + T], 'recall': m[6 + T:6 + 2 * T], 'fscore': m[6 + 2 * T:6 + 3 * T]}

        keys = ('cd', 'cd_l1', 'accuracy', 'completeness', 'normal_consistency', 'precision', 'recall', 'fscore')
        total = figures(sums[:W], n_samples)
        per_class = [figures(sums[(1 + c) * W:(2 + c) * W], class_n[c]) for c in range(C)]
        res = {k: None if total is None else total[k] for k in keys}
        for k in keys:
            res['class_' + k] = [None if f is None else f[k] for f in per_class]
        res.update(class_n=class_n, n_samples=n_samples, n_batches=n_batches, n_invalid=n_invalid,
                   thresholds=list(self.thresholds))
        return res

    def report(self, epoch=None, group=None):
        """Prints one line per class that occurred, then the total; a line for n_invalid when it is not zero.  Returns
        result()."""
        res = self.result(group)
        head = '\nEpoch %d\n' % epoch if epoch is not None else ''
        print(head + '=' * 30)

        def line(name, get):
            nc = get('normal_consistency')
            text = '%s \t\tsurface cd = %.6f, cd_l1 = %.6f, nc = %s' % (name, get('cd'), get('cd_l1'),
                                                                     'n/a' if nc is None else '%.4f' % nc)
            for t, tau in enumerate(self.thresholds):
                text += ', F@%g = %.4f (P %.4f, R %.4f)' % (tau, get('fscore')[t], get('precision')[t], get('recall')[t])
            print(text)

        for i, name in enumerate(self.class_names):
            if res['class_n'][i]:
                line(name, lambda k, i=i: res['class_' + k][i])
        print('=' * 30)
        if res['n_samples']:
            line('total', lambda k: res[k])
        else:
            print('total \t\tno samples')
        if res['n_invalid']:
            print('n_invalid = %d (class index outside [0, %d): in the total, in no class)' % (res['n_invalid'], self.C))
        return res


class VolumeEvaluationMeter:
    """Per-class volumetric IoU of an evaluation epoch, kept on the device (csrc/occupancy.hip):

        meter = VolumeEvaluationMeter(class_names, device, resolution=32)
        for data in dataloader:
            ...
            meter.update_primitives(params, kinds, gt_batch, data['class_index'], gt_xforms=view)
        meter.report(epoch)

    The prediction and the ground truth are asked "is x inside" at the same query points -- by default the resolution^3 cell
    centres of the cube `bounds`^3 (ops.grid_queries), or any `queries` fp32 [Q,3] -- and compared per sample:
        iou = #(pred and gt) / #(pred or gt), precision = #and / #pred, recall = #and / #gt, vol_pred = #pred / Q, vol_gt = #gt / Q
    each 0 where its denominator is 0; a sample whose union is empty counts in n_empty.  A primitive assembly is inside where
    any primitive's closed-form test holds (ops.primitive_occupancy); a triangle mesh where its generalized winding number
    exceeds 0.5 (ops.mesh_occupancy), which also serves meshes with holes and overlapping closed components.

    Like SurfaceEvaluationMeter, `update` makes no host synchronisation, can be captured into a HIP graph and is bit-equal
    from run to run; `result` is the ONE device-to-host copy of an epoch; the totals are SAMPLE-weighted; a class index
    outside [0, C) enters the totals, no class, and n_invalid."""

    def __init__(self, class_names, device, resolution=32, bounds=(-0.5, 0.5), queries=None):
        self.class_names = [str(c) for c in class_names]
        if not self.class_names:
            raise ValueError('VolumeEvaluationMeter needs at least one class name')
        self.C = len(self.class_names)
        self.device = torch.device(device)
        self.W = ops.VOLIOU_WIDTH
        if queries is None:
            self.resolution, self.bounds = int(resolution), (float(bounds[0]), float(bounds[1]))
            self.queries = ops.grid_queries(self.resolution, self.bounds[0], self.bounds[1], self.device)
        else:
            if (not isinstance(queries, torch.Tensor) or queries.dim() != 2 or queries.shape[1] != 3 or queries.shape[0] < 1
                    or queries.dtype != torch.float32):
                raise ValueError('queries must be a float32 tensor [Q,3], got %r' % (tuple(getattr(queries, 'shape', ())),))
            self.resolution, self.bounds = None, None
            self.queries = queries.detach().to(self.device).contiguous()
        self.state = ops.voliou_state(self.C, self.device)

    _class_index = EvaluationMeter._class_index

    @torch.no_grad()
    def update(self, occ_pred, occ_gt, class_indices):
        """One batch of occupancies uint8 [B,Q] on the device (non-zero = inside), class_indices [B] (a device tensor, a CPU
        tensor or a list).  Returns (rows [B,5] = iou, precision, recall, vol_pred, vol_gt; counts int32 [B,4] = and, or,
        prediction, ground truth) as device tensors."""
        if not (isinstance(occ_pred, torch.Tensor) and isinstance(occ_gt, torch.Tensor) and occ_pred.dim() == 2):
            raise ValueError('occ_pred and occ_gt uint8 [B,Q] expected')
        if not (occ_pred.is_cuda and occ_gt.is_cuda):
            raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path'
                               % occ_pred.device.type)
        return ops.voliou_step(occ_pred, occ_gt, self._class_index(class_indices, occ_pred.size(0)), self.state, self.C)

    def _gt_occupancy(self, gt_batch, gt_xforms, B):
        if not hasattr(gt_batch, 'face_counts'):
            raise TypeError('gt_batch must be a MeshBatch (MeshBatch.pack / MeshBatch.from_objs)')
        if len(gt_batch) != B:
            raise ValueError('%d ground-truth meshes for a batch of %d' % (len(gt_batch), B))
        return ops.mesh_occupancy(gt_batch, None, self.queries, gt_xforms)

    @torch.no_grad()
    def update_primitives(self, params, kinds, gt_batch, class_indices, gt_xforms=None):
        """One batch of predicted primitive assemblies: params [B,K,10], kinds [K]; gt_batch: a MeshBatch of B ground-truth
        meshes, gt_xforms [B,3,4] the affine map that brings them into the prediction's frame (view_center_xforms).
        ops.primitive_occupancy, ops.mesh_occupancy on the meter's queries, then `update`."""
        if not (isinstance(params, torch.Tensor) and params.dim() == 3):
            raise ValueError('params [B,K,10] expected')
        occ_gt = self._gt_occupancy(gt_batch, gt_xforms, params.size(0))
        occ_pred = ops.primitive_occupancy(params.detach().float(), kinds, self.queries)
        return self.update(occ_pred, occ_gt, class_indices)

    @torch.no_grad()
    def update_mesh(self, verts, faces, gt_batch, class_indices, gt_xforms=None):
        """One batch of predicted MESHES: verts [B,P,3], one faces [F,3] for the batch; the ground truth as in
        update_primitives.  ops.mesh_occupancy for both, then `update`.  Faces are wound counter-clockwise seen from outside
        (w = +1 inside); a mesh wound the other way has w = -1 inside and holds no point: pass faces.flip(1), as
        examples/eval_step.py does for the uv_sphere template."""
        if not (isinstance(verts, torch.Tensor) and verts.dim() == 3 and verts.size(-1) == 3):
            raise ValueError('verts [B,P,3] expected')
        occ_gt = self._gt_occupancy(gt_batch, gt_xforms, verts.size(0))
        occ_pred = ops.mesh_occupancy(verts.detach().float(), faces, self.queries)
        return self.update(occ_pred, occ_gt, class_indices)

    def reset(self):
        self.state.zero_()

    def load_state(self, state):
        """Replace the meter's state by a copy of `state` (a state tensor of the same number of classes, any device)."""
        ops.voliou_state_fields(state, self.C)
        self.state.copy_(state)

    @staticmethod
    def merge(state_a, state_b):
        """The state of two evaluations taken together: the field-wise sum of two state tensors of the same classes (sums
        as float64, counts as int64).  What result(group=...) does across ranks, without a process group; works on CPU
        tensors.  The number of classes follows from the size."""
        W = ops.VOLIOU_WIDTH
        if state_a.shape != state_b.shape or state_a.dim() != 1 or state_a.numel() < 2 * W + 5 or (state_a.numel() - 4 - W) % (W + 1):
            raise ValueError('merge needs two volumetric evaluation states of the same number of classes')
        C = (state_a.numel() - 4 - W) // (W + 1)
        out = torch.empty_like(state_a)
        (sa, na), (sb, nb), (so, no) = (ops.voliou_state_fields(t, C) for t in (state_a, state_b.to(state_a.device), out))
        torch.add(sa, sb, out=so)
        torch.add(na, nb, out=no)
        return out

    def result(self, group=None):
        """The epoch so far as plain Python.  Epoch figures 'iou', 'precision', 'recall', 'vol_pred', 'vol_gt' (None without
        samples); per class the same keys as 'class_*' lists, None for a class that never occurred; 'class_n', 'n_samples',
        'n_batches', 'n_empty', 'n_invalid'.  group: a torch.distributed process group whose ranks each evaluated a shard:
        their states are summed by one all-reduce first.  One device-to-host copy."""
        state = self.state if group is None else vdist.all_reduce_voliou_state(self.state, self.C, group)
        sums, counts = ops.voliou_state_fields(state.cpu(), self.C)
        sums, counts = sums.tolist(), counts.tolist()
        C, W, keys = self.C, self.W, ops.VOLIOU_COLUMNS
        n_samples, n_batches, n_empty, n_invalid, class_n = counts[0], counts[1], counts[2], counts[3], counts[4:]
        figures = lambda row, n: [v / n for v in row] if n else None
        total = figures(sums[:W], n_samples)
        per_class = [figures(sums[(1 + c) * W:(2 + c) * W], class_n[c]) for c in range(C)]
        res = {k: None if total is None else total[i] for i, k in enumerate(keys)}
        for i, k in enumerate(keys):
            res['class_' + k] = [None if f is None else f[i] for f in per_class]
        res.update(class_n=class_n, n_samples=n_samples, n_batches=n_batches, n_empty=n_empty, n_invalid=n_invalid)
        return res

    def report(self, epoch=None, group=None):
        """Prints one line per class that occurred, then the total; a line each for n_empty and n_invalid when not zero.
        Returns result()."""
        res = self.result(group)
        head = '\nEpoch %d\n' % epoch if epoch is not None else ''
        print(head + '=' * 30)

        def line(name, get):
            print('%s \t\tvolume iou = %.4f (P %.4f, R %.4f), vol_pred = %.4f, vol_gt = %.4f'
                  % (name, get('iou'), get('precision'), get('recall'), get('vol_pred'), get('vol_gt')))

        for i, name in enumerate(self.class_names):
            if res['class_n'][i]:
                line(name, lambda k, i=i: res['class_' + k][i])
        print('=' * 30)
        if res['n_samples']:
            line('total', lambda k: res[k])
        else:
            print('total \t\tno samples')
        if res['n_empty']:
            print('n_empty = %d (neither the prediction nor the ground truth holds a query point: iou 0)' % res['n_empty'])
        if res['n_invalid']:
            print('n_invalid = %d (class index outside [0, %d): in the total, in no class)' % (res['n_invalid'], self.C))
        return res

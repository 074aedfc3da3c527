"""Capture tests/golden/g9_eval.npz from the reference's own modules/loss/chamfer_distance.py on the CPU.

    python tools/make_golden_eval.py /path/to/reference

chamfer_distance.py imports only torch and `config`; a stub `config` module (DEVICE = 'cpu', CD_W1 = CD_W2 = 1.0 as the
reference's config.py:11-12 has them) is put in sys.modules so that it loads.  Only data is written (allow_pickle=False):
the batches (pred, gt, class_index, concatenated; batch_sizes splits them) and what the reference's
ChamferDistanceLoss()(pred, gt, each_batch=True) gives for them, run through the bookkeeping of an evaluation epoch
(test.py:104-108, :126-133) in Python floats: the per-sample losses (fp32), the per-class sums and the sum of the batch
means as float64, the class counts, the number of batches.

The class indices are chosen so that the fixture holds a class that never occurs (12), a class hit several times within one
batch (3, four times in batch 2) and a class hit in every batch (0).  The last batch is short (5 of 8).

The EMD half is not captured: the reference's auction is a CUDA extension; its expected values come from this project's own
auction (tests/test_evaluation.py)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g9_eval.npz')
SIZE_CAP = 402312                        # the largest fixture committed before this one
C, N, M = 13, 128, 96
BATCH_SIZES = (8, 8, 8, 8, 8, 8, 5)


def load_reference_chamfer(ref_root):
    cfg = types.ModuleType('config')
    cfg.DEVICE = 'cpu'
    cfg.CD_W1, cfg.CD_W2 = 1.0, 1.0
    sys.modules['config'] = cfg
    spec = importlib.util.spec_from_file_location('ref_chamfer', os.path.join(ref_root, 'modules', 'loss', 'chamfer_distance.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    g = torch.Generator().manual_seed(909)
    total = sum(BATCH_SIZES)
    gt = torch.rand(total, M, 3, generator=g) - 0.5
    # predictions of varying quality: the ground truth's neighbourhood at a per-sample noise level, so that classes differ
    noise = torch.rand(total, 1, 1, generator=g) * 0.2 + 0.01
    pick = torch.randint(0, M, (total, N), generator=g)
    pred = torch.gather(gt, 1, pick[..., None].expand(-1, -1, 3)) + noise * torch.randn(total, N, 3, generator=g)
    cls = torch.randint(1, 12, (total,), generator=g)            # classes 1..11; 12 never occurs
    cls[cls == 3] = 4                                            # class 3 only where it is placed below
    lo = 0
    for k, b in enumerate(BATCH_SIZES):
        cls[lo] = 0                                              # class 0 in every batch
        if k == 2:
            cls[lo + 2:lo + 6] = 3                               # class 3 four times within one batch
        lo += b
    return pred, gt, cls


def main(ref_root):
    ref = load_reference_chamfer(ref_root)
    loss_func = ref.ChamferDistanceLoss()
    pred, gt, cls = inputs()
    # the bookkeeping of test.py:83-85, :104-108, :126-133 on the reference's own per-sample losses, over each batch's real size
    total, n = 0.0, 0
    class_sum = [0.0] * C
    class_n = [0] * C
    loss_b = []
    lo = 0
    for b in BATCH_SIZES:
        with torch.no_grad():
            cd = loss_func(pred[lo:lo + b], gt[lo:lo + b], each_batch=True) * 1.0          # L_VIEW_CD = 1.0 (config.py:13)
        total += cd.mean().item()
        for i in range(b):
            class_sum[int(cls[lo + i])] += cd[i].item()
            class_n[int(cls[lo + i])] += 1
        n += 1
        loss_b.append(cd)
        lo += b
    class_n_arr = np.array(class_n, np.int64)
    assert class_n_arr[12] == 0 and class_n_arr[3] == 4 and class_n_arr[0] >= len(BATCH_SIZES)
    data = dict(pred=pred.numpy(), gt=gt.numpy(), class_index=cls.numpy().astype(np.int64),
                batch_sizes=np.array(BATCH_SIZES, np.int64), num_classes=np.int64(C),
                loss_b=torch.cat(loss_b).numpy(), class_sum=np.array(class_sum, np.float64), class_n=class_n_arr,
                total_sum=np.float64(total), n_batches=np.int64(n), total=np.float64(total / n))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size <= SIZE_CAP, size
    print('wrote %s: %d bytes; class_n %s; total %.6f' % (OUT, size, class_n, total / n))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('VPN_REFERENCE', ''))

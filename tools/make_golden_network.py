"""Record what tests/test_network_cpu.py needs to know about the reference's networks into tests/golden/g11_network.npz:
the state_dict names and shapes of the FC heads (VPNetOneRes, VPNetTwoRes) and of SDNet's deform stack with IS_DROPOUT
off and on, and one small case of restrict_range -> split -> restrict_volumes with IS_SIGMOID on and off.  Names, shapes
and a few dozen floats; no weights.

    python tools/make_golden_network.py --reference /path/to/reference

The reference's model files import torchvision, which is not a dependency here: a stub `torchvision.models.resnet18`
that returns an empty module goes into sys.modules first (the heads do not depend on the trunk).  Run where the reference
is checked out; the tests read only the fixture."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(ref, name):
    path = os.path.join(ref, 'modules', 'network', name + '.py')
    spec = importlib.util.spec_from_file_location('ref_' + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def head_entries(model):
    sd = model.state_dict()
    keys = [k for k in sd if '_fc.' in k or '.deform.' in k]
    return keys, [list(sd[k].shape) for k in keys]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'g11_network.npz'))
    args = ap.parse_args()
    tv, tvm = types.ModuleType('torchvision'), types.ModuleType('torchvision.models')
    tvm.resnet18 = lambda pretrained=False: nn.Module()
    tv.models = tvm
    sys.modules['torchvision'], sys.modules['torchvision.models'] = tv, tvm
    sys.path.insert(0, args.reference)
    mods = {'one': load(args.reference, 'vpnet_one_resnet'), 'two': load(args.reference, 'vpnet_two_resnet'),
            'sd': load(args.reference, 'sdnet')}
    cls = {'one': 'VPNetOneRes', 'two': 'VPNetTwoRes', 'sd': 'SDNet'}
    out = {}
    for tag, mod in mods.items():
        for drop in (0, 1):
            if tag != 'sd':
                mod.IS_DROPOUT = bool(drop)
            keys, shapes = head_entries(getattr(mod, cls[tag])())
            out['%s_drop%d_names' % (tag, drop)] = np.array(keys)
            out['%s_drop%d_shapes' % (tag, drop)] = np.array([s + [0] * (2 - len(s)) for s in shapes], dtype=np.int64)   # bias: (n, 0)
    one = mods['one']
    out['vp_num'] = np.array(one.CUBOID_NUM + one.SPHERE_NUM + one.CONE_NUM)
    out['clamp'] = np.array([one.VP_CLAMP_MIN, one.VP_CLAMP_MAX], dtype=np.float64)
    out['volume_restrict'] = np.array(one.VOLUME_RESTRICT, dtype=np.float64)
    g = torch.Generator().manual_seed(11)
    B, K = 2, 3
    v, q, t = [(torch.rand(B, n * K, generator=g) * 4 - 2) for n in (3, 4, 3)]      # crosses every clamp bound
    out['raw_volumes'], out['raw_rotates'], out['raw_translates'] = v.numpy(), q.numpy(), t.numpy()
    for sig in (0, 1):
        one.IS_SIGMOID = bool(sig)
        with torch.no_grad():
            a, b, c = one.VPNetOneRes.restrict_range(v.clone(), q.clone(), t.clone())
            a = one.VPNetOneRes.restrict_volumes(list(a.split(3, dim=1)))
            b, c = list(b.split(4, dim=1)), list(c.split(3, dim=1))
        out['sig%d_volumes' % sig] = torch.stack(a, 1).numpy()          # (B,K,3)
        out['sig%d_rotates' % sig] = torch.stack(b, 1).numpy()
        out['sig%d_translates' % sig] = torch.stack(c, 1).numpy()
    np.savez(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()

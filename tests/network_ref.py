"""CPU restatement of the FC heads (csrc/fcstack.hip) in plain torch: F.linear chains in float64, dropout with explicit
keep masks, and what follows the last layer (tanh, or restrict_range -> split -> restrict_volumes into packed rows).
Everything is differentiable, so gradients come from autograd in float64; callers round to float32 where they compare.
Independent of the package and of oracle/: only torch."""
import torch
import torch.nn.functional as F


def stack(xs, params, masks=None, p=0.5):
    """xs: one (B,in) tensor per group; params: per group a list of (weight [out,in], bias [out]); masks: per group a
    list of keep masks (B,out) for layers 0..L-2 (None: no dropout).  Returns the raw outputs, float64."""
    outs = []
    for g, (x, layers) in enumerate(zip(xs, params)):
        h = x.double()
        for l, (w, b) in enumerate(layers):
            h = F.linear(h, w.double(), b.double())
            if masks is not None and l < len(layers) - 1:
                h = h * masks[g][l].double() / (1.0 - p)
        outs.append(h)
    return outs


def restrict_range(volumes, rotates, translates, is_sigmoid, clamp_min, clamp_max):
    if is_sigmoid:
        return torch.sigmoid(volumes) + 0.1, torch.sigmoid(rotates), torch.tanh(translates)
    return (torch.clamp(volumes, min=clamp_min + 1e-8, max=clamp_max), torch.clamp(rotates, min=-1, max=1),
            torch.clamp(translates, min=-1, max=1))


def vp_pack(volumes, rotates, translates, is_sigmoid, clamp_min, clamp_max, volume_restrict):
    """Raw (B,3K), (B,4K), (B,3K) -> packed (B,K,10): (v / restrict | q | t) of primitive k in row k."""
    v, q, t = restrict_range(volumes, rotates, translates, is_sigmoid, clamp_min, clamp_max)
    B, K = v.shape[0], v.shape[1] // 3
    r = torch.as_tensor(volume_restrict, dtype=v.dtype)
    return torch.cat([v.reshape(B, K, 3) / r, q.reshape(B, K, 4), t.reshape(B, K, 3)], dim=2)

"""The GCN's collapsed layer pairs for the tests: the meshes both test files share, the float64 statement of a
pair in both forms (two layers in a row; one product, then two propagations) through tests/gcn_ref.py, the block partition
by brute force, and the skinny projection."""
import torch

import gcn_input_ref as G
import gcn_ref as R


def _strip(n):
    """Triangle strip over n >= 3 consecutive vertices: connected, every edge at most 2 apart."""
    return torch.tensor([[i, i + 1, i + 2] for i in range(n - 2)])


def meshes(limit):
    """name -> (faces, n); `limit` = ops.GCN_HOP2_MAX_ROWS."""
    irr, _ = G.irregular_mesh()                                       # 9 vertices, vertex 8 in no face
    tri = torch.tensor([[0, 1, 2]])
    even = torch.tensor([[0, 2, 4], [2, 4, 6], [4, 6, 8], [6, 8, 10]])
    return {
        'two_irregular_and_lone': (torch.cat([irr, irr + 9]), 19),    # closed ranges 8, 1, 8, 1, 1
        'single_vertex': (torch.zeros(0, 3, dtype=torch.long), 1),
        'triangles_70': (torch.cat([tri + 3 * k for k in range(70)]), 210),
        'interleaved': (torch.cat([even, even + 1]), 12),             # two components, one closed range
        'clique_70': (torch.tensor([[i, j, j] for i in range(70) for j in range(i + 1, 70)]), 70),   # 4900 entries of A_hat
        'strip_max': (_strip(limit), limit),
        'strip_max_plus_1': (_strip(limit + 1), limit + 1),           # no table: the fallback
    }


def closed_ranges(edges, n):
    """Brute force: i starts a closed range when no edge (a, b) has min < i <= max."""
    e = [(min(a, b), max(a, b)) for a, b in edges.tolist()]
    return [i for i in range(n) if not any(a < i <= b for a, b in e)]


def check_table(starts, edges, n, limit):
    """A block table covers [0, n) in ascending blocks of 1..limit rows whose starts no edge crosses, and is greedy: a block
    plus the closed range that follows it would exceed the limit."""
    assert starts[0] == 0 and starts[-1] == n and all(0 < b - a <= limit for a, b in zip(starts, starts[1:])), starts
    closed = closed_ranges(edges, n) + [n]
    assert set(starts) <= set(closed), (starts, closed)
    for a, b in zip(starts[:-2], starts[1:-1]):
        nxt = closed[closed.index(b) + 1]
        assert nxt - a > limit, (a, b, nxt)


def pair_plain(x, ta, tb, ba, bb, norm):
    """conv_b(conv_a(x)) as GCNModel states it: two layers in a row."""
    return R.aggregate(R.aggregate(x @ ta, norm, ba) @ tb, norm, bb)


def pair_collapsed(x, ta, tb, ba, bb, norm):
    """The same map with one product: A(A(x Theta_a Theta_b) + b_a Theta_b) + b_b."""
    return R.aggregate(R.aggregate(x @ (ta @ tb), norm, ba @ tb), norm, bb)


def aggregate2(h, u, b, norm, mask=None, relu=False):
    """A(A h + u) + b in the dtype of h; the ReLU by `mask` (the decisions another implementation took) when given."""
    y = R.aggregate(R.aggregate(h, norm, u), norm, b)
    if mask is not None:
        return y * mask.to(y.dtype)
    return y.relu() if relu else y


def project(x, theta):
    return x @ theta

"""The ordered entry-point calls of the two fused loss nodes, as _lib.KernelTimer records them.  README's "4 launches" of
the hot path and "9 forward, 1 backward" of the training step rest on these lists; they were recorded from the code before
ops.py shared the hot-path launches between the two nodes, not written from the code they check."""
import pytest
import torch

from conftest import ROOT  # noqa: F401
from test_trainstep import _batch

DEV = 'cuda'

HOT_PATH_CALLS = ['vpn_hotpath_sample_fwd', 'vpn_hotpath_chamfer_fwd', 'vpn_raster_total_fwd_fin', 'vpn_hotpath_bwd']
TRAIN_STEP_CALLS = ['vpn_hotpath_sample_fwd', 'vpn_emd_fwd_ex', 'vpn_hotpath_chamfer_fwd', 'vpn_raster_total_fwd_fin',
                    'vpn_camera_transform_fwd', 'vpn_chamfer_fwd_ws', 'vpn_camera_matrix', 'vpn_vpdiv_fwd',
                    'vpn_trainstep_finalize', 'vpn_trainstep_bwd']


@pytest.fixture
def default_switches():
    """The launch order under the shipped defaults, whatever the environment of the test run sets."""
    from vpn_amd import ops
    old = ops.TILE_ORDER, ops.CONCURRENT_BRANCHES
    ops.TILE_ORDER, ops.CONCURRENT_BRANCHES = True, False
    yield
    ops.TILE_ORDER, ops.CONCURRENT_BRANCHES = old


def _recorded(step):
    import vpn_amd
    with vpn_amd._lib.KernelTimer() as timer:
        step()
    torch.cuda.synchronize()
    names = [name for name, _a, _b in timer.records]
    print(names)
    return names


@pytest.mark.gpu
def test_hot_path_node_call_order(default_switches):
    """Fused Chamfer features and a tile rider that fits (K = 4, 2 x 2 tiles): sampler, scan + rider, raster +
    finalisation, one backward launch."""
    import vpn_amd
    B, K, n, M, H, W = 2, 4, 160, 512, 32, 32
    assert vpn_amd._lib.lib().vpn_hotpath_fused_features(B, K, n, M) == 1
    g = torch.Generator().manual_seed(11)
    params = _batch(B, K, n, H, 11, DEV)[0].requires_grad_(True)
    cam = torch.tensor([[1.0, 0.0, 0.0]]).expand(B, 3).contiguous().to(DEV)
    gt_points = (torch.rand(B, M, 3, generator=g) - 0.5).to(DEV)
    gt_sil = (torch.rand(B, 1, H, W, generator=g) > 0.5).float().to(DEV)
    gt_depth = (2.0 - torch.rand(B, H, W, generator=g)).to(DEV)
    cfg = vpn_amd.config

    def step():
        out = vpn_amd.HotPathLossFunction.apply(params, vpn_amd.kinds_tensor([1, 0, 0, 0], DEV), cam, gt_points, gt_sil, gt_depth,
                                                n, 7, 0, H, W, cfg.RASTER_SIGMA, cfg.RASTER_GAMMA, cfg.RASTER_Z_FAR, 1.0, 1.0, 1.0)
        out[2].backward()
    assert _recorded(step) == HOT_PATH_CALLS


@pytest.mark.gpu
def test_train_step_node_call_order(default_switches):
    """All five weights non-zero: the hot path's three launches with the auction between the sampler and the scan, the
    object-centred cloud, the VP-diversity neighbours, the reduction, one backward launch."""
    import vpn_amd
    B, K, n, H = 3, 16, 32, 64
    assert vpn_amd._lib.lib().vpn_hotpath_fused_features(B, K, n, K * n) == 1
    params, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles = _batch(B, K, n, H, 5, DEV)
    params.requires_grad_(True)
    kinds = vpn_amd.kinds_tensor([0] * K, DEV)

    def step():
        out = vpn_amd.TrainStepLossFunction.apply(params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, n, 77, 0,
                                                  H, H, (1.0, 0.7, 1.0, 0.1, 1.0))
        out[5].backward()
    assert _recorded(step) == TRAIN_STEP_CALLS

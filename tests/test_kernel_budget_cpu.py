"""The EMD auction runs BESIDE the training step's other kernels: one workgroup per CU that must leave them
registers and LDS.  Measured in round 4: with the auction at 94-96 VGPRs (a build with one more code path in the kernel)
instead of 86 the co-running raster and the second Chamfer scan stretched to 480 / 256 us, the main branch became as long
as the auction and the C5 step went from 0.90 to 1.02 ms.  This test compiles emd.hip the way build.py does and holds the
kernel to the budget the overlap was measured with."""
from kernel_resources import kernel_resources


def _resources(src, kernel):
    rows = kernel_resources(src)
    hits = [v for k, v in rows.items() if kernel in k]
    assert len(hits) == 1, (kernel, list(rows))
    return hits[0]


def test_emd_auction_kernel_leaves_room_for_the_step():
    r = _resources('emd.hip', 'emd_auction_team_kernel')
    # four waves per SIMD at <= 88 VGPRs leave 160 of the 512 registers of a SIMD lane; no scratch
    assert r['VGPRs'] + r.get('AGPRs', 0) <= 88, r
    assert r['ScratchSize'] == 0, r
    # static LDS + the dynamic part at n = 2048, G = 4 (32 n + 18 n / G + the balanced form's lists) must leave the scan
    # kernel's 30 792 bytes of a CU's 160 KB
    dynamic = 32 * 2048 + 18 * 512 + 51728
    assert r['LDS'] + dynamic + 30792 <= 160 * 1024, (r, dynamic)

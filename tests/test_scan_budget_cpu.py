"""The fp16 Chamfer scan `chamfer_nn_mfma_kernel<2>` is more than half of the C3 step and runs at the edge of its
budget: six waves per SIMD need <= 80 VGPRs, 4 bytes of scratch were measured at 10-20 us, and three
workgroups of eight waves must share a CU's LDS.  In the training step it also runs beside the EMD auction, which
leaves it what tests/test_kernel_budget_cpu.py states.  This test compiles chamfer.hip the way build.py does and holds
the kernel, candidate prologue included, to that budget."""
from test_kernel_budget_cpu import _resources

LDS_PER_CU = 160 * 1024


def test_fp16_scan_kernel_budget():
    r = _resources('chamfer.hip', 'chamfer_nn_mfma_kernelILi2E')
    assert r['VGPRs'] + r.get('AGPRs', 0) <= 80, r
    assert r['ScratchSize'] == 0, r
    assert 3 * r['LDS'] <= LDS_PER_CU, r
    # beside one auction workgroup at n = 2048, G = 4 (its static 4640 bytes + the dynamic part: see the auction's test)
    assert r['LDS'] + 4640 + 32 * 2048 + 18 * 512 + 51728 <= LDS_PER_CU, r

"""Per-kernel register / LDS / occupancy table of one .hip file as build.py compiles it (hipcc -Rpass-analysis).
    python tools/kres.py chamfer.hip [filter]"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
from kernel_resources import kernel_resources  # noqa: E402

flt = sys.argv[2] if len(sys.argv) > 2 else ''
for mangled, v in kernel_resources(sys.argv[1]).items():
    k = subprocess.run(['c++filt', mangled], capture_output=True, text=True).stdout.strip().split('(')[0]
    if flt in k:
        print('%-60s sgpr %-4s vgpr %-4s agpr %-3s scratch %-4s occ %-2s lds %s' % (k[-60:], v.get('TotalSGPRs'), v.get('VGPRs'), v.get('AGPRs'),
              v.get('ScratchSize'), v.get('Occupancy'), v.get('LDS')))

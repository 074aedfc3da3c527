"""What hipcc reports about the kernels of one csrc/*.hip file, compiled the way build.py compiles it
(-Rpass-analysis=kernel-resource-usage).  Used by the resource tests and by tools/kres.py."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REMARK = re.compile(r'remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|'
                     r'LDS Size \[bytes/block\]): (\S+)')


def load_build():
    """volumetric-primitives-net_amd/build.py as a module (the directory's name is no Python identifier)."""
    spec = importlib.util.spec_from_file_location('vpn_build', os.path.join(ROOT, 'volumetric-primitives-net_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def kernel_resources(src):
    """{mangled kernel name: {'TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS': int}} of csrc/`src`, in the
    compiler's order.  A compile that fails is an AssertionError with the end of its messages."""
    b = load_build()
    cmd = [b.hipcc()] + b.COMMON + b.PER_FILE.get(src, []) + ['-c', os.path.join(b.CSRC, src), '-o', os.devnull,
                                                               '-Rpass-analysis=kernel-resource-usage']
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    cur, rows = None, {}
    for line in run.stderr.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            cur = rows[m.group(2)] = {}
        elif cur is not None:
            cur[m.group(1).split(' ')[0]] = int(m.group(2))
    return rows

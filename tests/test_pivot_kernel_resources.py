"""Register/scratch budget of the pivot spread kernel (compile-time check, no
GPU): csrc/kernels/pivot.hip reads the per-output pointers and fills of up to
16 outputs from a by-value argument struct. Indexed with a uniform loop
counter the struct stays in the argument segment; a copy of it in private
memory would be scratch, and all sixteen outputs' pointers and fills held in
registers at once would spill. The file is compiled for gfx950 with hipcc's
resource-usage remarks, as tests/test_unique_kernel_resources.py does for the
distinct-rows kernels."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
KERNELS = ("pivot_spread_kernel",)


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_pivot_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I", os.path.join(REPO, "csrc"),
           "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
           os.path.join(REPO, "csrc", "kernels", "pivot.hip"), "-o", str(tmp_path / "k.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                kernels[cur][key] = int(m.group(1))
    assert len(kernels) == len(KERNELS), sorted(kernels)                 # each of the file's kernels is checked
    for name in KERNELS:
        found = [v for k, v in kernels.items() if name in k]
        assert len(found) == 1, (name, sorted(kernels))
        assert found[0] == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, (name, found[0])

"""Register/scratch budget of the grouped-statistics kernels (compile-time
check, no GPU).

group_moments keeps a six-field record, four rows in flight and a dtype switch
per lane; a loop the unroller gives up on, or an array indexed with a runtime
value, would put that in scratch and turn a gather-bound kernel into a
scratch-bound one. hipcc's resource-usage remarks show it as ScratchSize > 0,
so csrc/kernels/group_stats.hip is compiled for gfx950 here (the command line
of tests/test_kernel_resources.py) and every kernel in it is checked."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
KERNELS = ("group_chunk_count_kernel", "group_moments_kernel", "group_fold_kernel", "merge_group_records_kernel",
           "group_results_kernel")


def _resources(src, tmp_path):
    out = tmp_path / "k.o"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=fast",
           "-munsafe-fp-atomics", "-I", os.path.join(REPO, "csrc"), "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(REPO, "csrc", "kernels", src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and cur:
                kernels[cur].setdefault(key, int(m.group(1)))
    return kernels


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_group_stats_kernels_use_no_scratch(tmp_path):
    kernels = _resources("group_stats.hip", tmp_path)
    print(kernels)
    for name in KERNELS:
        assert any(name in k for k in kernels), f"{name} not found in group_stats.hip: {sorted(kernels)}"
    bad = {k: v for k, v in kernels.items() if v.get("ScratchSize [bytes/lane]", 0) or v.get("VGPRs Spill", 0)}
    assert not bad, f"grouped-statistics kernels spilling to scratch: {bad}"

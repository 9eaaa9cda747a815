"""Register/scratch budget of the pair-statistics kernels (compile-time check,
no GPU).

The dense pass keeps two runs of sixteen f64 values, a seven-field record and
two dtype switches per lane, the grouped pass four gathered rows of both
columns: an array indexed with a runtime value, or a loop the unroller gives
up on, would put that in scratch. hipcc's resource-usage remarks show it as
ScratchSize > 0, so csrc/kernels/stats.hip and csrc/kernels/group_stats.hip
are compiled for gfx950 here (the command line of
tests/test_group_stats_resources.py) and every new kernel is checked."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
KERNELS = {"stats.hip": ("pair_moments_partial_kernel", "pair_moments_final_kernel"),
           "group_stats.hip": ("group_pair_moments_kernel", "group_pair_fold_kernel", "merge_pair_records_kernel",
                               "pair_results_kernel")}


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
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_pair_kernels_use_no_scratch(src, tmp_path):
    kernels = _resources(src, tmp_path)
    print(kernels)
    for name in KERNELS[src]:
        found = [k for k in kernels if name in k]
        assert found, f"{name} not found in {src}: {sorted(kernels)}"
        for k in found:
            v = kernels[k]
            assert "ScratchSize [bytes/lane]" in v and "VGPRs Spill" in v, (k, v)
            assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, f"{k} spills to scratch: {v}"

"""The compiler's per-kernel resource-usage remarks (-Rpass-analysis=kernel-resource-usage) of one csrc/*.hip file at the product flags:
what the register-budget tests (test_color_pts_resources.py, test_sdf_resources.py) assert on.  No GPU needed."""
import importlib
import os
import re
import shutil
import subprocess

build = importlib.import_module("one-2-3-45_amd.build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HAVE_HIPCC = bool(shutil.which(HIPCC)) or os.path.exists(HIPCC)


def kernel_usage(source, name_pattern, key, tmp_path):
    """Compile csrc/``source`` for the device only.  -> {key(match): {"VGPRs", "AGPRs", "ScratchSize", "Occupancy", "LDS"}} for every kernel whose
    mangled name matches ``name_pattern``."""
    src = os.path.join(build.CSRC, source)
    cmd = [HIPCC] + build.FLAGS + build.EXTRA_FLAGS.get(source, []) + ["--offload-device-only", "-c", src, "-o", str(tmp_path / (source + ".o")),
                                                               "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: " + name_pattern, line)
        if m:
            cur = key(m)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            out[cur].setdefault(m.group(1).split(" ")[0], int(m.group(2)))
        elif "Function Name:" in line:
            cur = None
    return out

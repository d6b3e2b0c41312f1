"""The compiler's own resource remarks of one HIP source, for the test_*_resources.py files: compiled with the project's flags and
-Rpass-analysis=kernel-resource-usage (no GPU needed, only hipcc), parsed once, here."""
import os
import re
import shutil
import subprocess


def hipcc():
    from forge_amd import build
    try:
        return build.hipcc()
    except RuntimeError:
        return shutil.which("hipcc")


def kernel_remarks(src, tmp_dir, name_filter=None):
    """{mangled kernel name: {"VGPRs", "AGPRs", "Occupancy", "LDS Size", "ScratchSize", "VGPRs Spill", "SGPRs Spill", ...: int}} of every kernel of `src`
    whose mangled name contains `name_filter` (None: all). None when there is no hipcc."""
    cc = hipcc()
    if not cc:
        return None
    from forge_amd import build
    obj = os.path.join(str(tmp_dir), os.path.basename(src) + ".o")
    p = subprocess.run([cc] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o", obj],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    out, cur = {}, None
    for line in p.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:.*?\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in out.items() if name_filter is None or name_filter in k}

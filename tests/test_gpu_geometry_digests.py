"""The geometry kernels and the image metrics claim the same bits everywhere: tools/geometry_digest.py hashes every output tensor of a fixed set of
calls, and tests/golden/geometry_digests.json is that listing as the commit before the kernels' shared header (csrc/geom_common.h) produced it on the
MI355X. A refactor of these files must reproduce it; a change that is meant to alter an output regenerates the file and says so. One entry reaches
further than these files: "image/lpips" is the whole seeded LPIPS module, so it also moves with the convolution trunk and with torch's seeded
CPU generator; when only that entry differs, look there first."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_outputs_match_the_pinned_digests():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import geometry_digest
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    with open(os.path.join(ROOT, "tests", "golden", "geometry_digests.json")) as fh:
        want = json.load(fh)
    got = geometry_digest.digests()
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, "%d of %d tensors differ from the pinned bits: %s" % (len(differ), len(want), differ[:20])

"""CPU: the host half of the photograph ingest (include/forge_hip.h section h) - the coefficient tables of libforge_hip.so against the tables stored
with the Pillow golden, the refusals, and the numpy restatement (tests/ingest_cases.py) against every golden case, byte for byte."""
import ctypes

import numpy as np
import pytest

import ingest_cases as ic
from forge_amd import _lib

EINVAL = -1


@pytest.fixture(scope="module")
def gold(golden):
    return golden("ingest_pillow")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def library_table(n_in, n_out):
    L = _lib.lib()
    K = L.forge_resample_taps(n_in, n_out)
    assert K > 0
    first, count, k = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32), np.full((n_out, K), -7, np.int32)
    assert L.forge_resample_coeffs(n_in, n_out, _p(first), _p(count), _p(k)) == 0
    return first, count, k


@pytest.mark.parametrize("n_in,n_out", ic.TABLES)
def test_resample_coeffs_match_the_golden_tables(built_lib, gold, n_in, n_out):
    first, count, k = library_table(n_in, n_out)
    pre = "table/%d_%d/" % (n_in, n_out)
    assert np.array_equal(first, gold[pre + "first"]) and np.array_equal(count, gold[pre + "count"])
    assert k.shape == gold[pre + "k"].shape and np.array_equal(k, gold[pre + "k"])
    assert (k[np.arange(k.shape[1])[None] >= count[:, None]] == 0).all()                       # rows are zero-padded
    assert np.abs(k.sum(axis=1) - (1 << ic.PRECISION_BITS)).max() <= k.shape[1]                # each row sums to 1 up to its roundings


def test_resample_taps_and_nearest(built_lib):
    L = _lib.lib()
    assert L.forge_resample_taps(301, 32) == 57 and L.forge_resample_taps(5, 16) == 5 and L.forge_resample_taps(4100, 8) == 3075
    assert L.forge_resample_taps(5000, 16) == 1875 and L.forge_resample_taps(3024, 256) == 71 and L.forge_resample_taps(8, 8) == 6
    for n_in, n_out in ((6, 9), (10, 9), (2, 7), (301, 32), (5, 16), (800, 256), (1, 4), (4100, 8)):
        f, c, k = library_table(n_in, n_out)
        rf, rc, rk = ic.coeffs(n_in, n_out)
        assert np.array_equal(f, rf) and np.array_equal(c, rc) and np.array_equal(k, rk), (n_in, n_out)
        idx = np.full(n_out, -7, np.int32)
        assert L.forge_resample_nearest(n_in, n_out, _p(idx)) == 0
        assert np.array_equal(idx, ic.nearest(n_in, n_out)), (n_in, n_out)
    # the running sum and floor((i + 0.5) n_in / n_out) part ways where a tap lands on an integer; Pillow keeps the running sum
    i = np.arange(7)
    assert not np.array_equal(ic.nearest(2, 7), ((2 * i + 1) * 2) // 14)


def test_refusals(built_lib):
    L = _lib.lib()
    buf = np.zeros(64, np.int32)
    for n_in, n_out in ((0, 4), (4, 0), (-3, 4), (4, -1)):
        assert L.forge_resample_taps(n_in, n_out) == EINVAL and b"non-positive" in L.forge_last_error()
        assert L.forge_resample_coeffs(n_in, n_out, _p(buf), _p(buf), _p(buf)) == EINVAL
        assert L.forge_resample_nearest(n_in, n_out, _p(buf)) == EINVAL
    assert L.forge_resample_coeffs(4, 4, None, _p(buf), _p(buf)) == EINVAL and b"null pointer" in L.forge_last_error()
    assert L.forge_resample_nearest(4, 4, None) == EINVAL
    assert (buf == 0).all()
    # the device entry refuses before any launch (no GPU here): the pointers are never dereferenced
    fake = 0x1000
    call = lambda src=fake, N=1, H=8, W=8, C=4, istr=256, rstr=32, tx=fake, Kx=1, ty=fake, Ky=1, Ho=4, Wo=4, bg=0, ws=fake, wsb=1 << 20: L.forge_ingest_rgba8(
        src, N, H, W, C, istr, rstr, tx, Kx, ty, Ky, Ho, Wo, bg, ws, wsb, fake, fake, fake, None)
    for kw in (dict(src=None), dict(tx=None), dict(ty=None), dict(ws=None), dict(N=0), dict(H=0), dict(W=-1), dict(Ho=0), dict(Wo=0), dict(Kx=0),
               dict(C=2), dict(C=5), dict(bg=3), dict(bg=-1), dict(rstr=31), dict(N=2, istr=255), dict(wsb=8 * 4 * 4 - 1), dict(ws=fake + 2)):
        assert call(**kw) == EINVAL, kw
    assert call(H=1 << 20, rstr=1 << 12, wsb=1 << 40) == -2 and b"32-bit" in L.forge_last_error()          # FORGE_ESHAPE: 2^32 bytes per image
    assert call(H=1 << 20, W=4, rstr=16, Wo=1 << 10, wsb=1 << 40) == -2                                       # ... the intermediate


@pytest.mark.parametrize("case", ic.CASES, ids=[c[0] for c in ic.CASES])
def test_restatement_matches_every_golden_case(gold, case):
    name, H, W, Ho, Wo = case
    rgba = ic.source(name, H, W)
    clips = [0, 0]
    for ch in (3, 4):
        for bg in ic.BACKGROUNDS:
            b, f, m = ic.ingest(np.ascontiguousarray(rgba[:, :, :ch]), Ho, Wo, bg, clips)
            want = gold[ic.key(name, ch, bg) + "/bytes"]
            assert b.shape == (Ho, Wo, 3) == want.shape and int((b != want).sum()) == 0, (ch, bg)
            assert np.array_equal(m[0], gold[ic.key(name, ch, bg) + "/mask"].astype(np.float32)), (ch, bg)
            if ch == 4 or name == "h7w5_4":
                assert 0.0 < m.mean() < 1.0                                                        # the mask has both values
    if name in ic.NOISE_CASES:
        assert min(clips) > 0                                                                      # the clip fires at both ends
    if name == ic.ALPHA_CASE:
        assert set(np.unique(rgba[..., 3])) == {0, 1, 128, 255}
        assert not np.array_equal(gold[ic.key(name, 4, "white") + "/bytes"], gold[ic.key(name, 4, "black") + "/bytes"])
        assert not np.array_equal(gold[ic.key(name, 4, "premasked") + "/bytes"], gold[ic.key(name, 4, "black") + "/bytes"])


def test_float_rule_on_all_bytes():
    b = np.arange(256, dtype=np.uint8)
    want = (b.astype(np.float64) / 255.0).astype(np.float32)                                       # what the loaders' `/ 255.0` and `.float()` give
    assert np.array_equal((b.astype(np.float32) / np.float32(255.0)).view(np.int32), want.view(np.int32))
    _, f, _ = ic.ingest(np.dstack([b.reshape(16, 16)] * 3 + [np.full((16, 16), 255, np.uint8)]), 16, 16, "white")
    assert np.array_equal(f[0].reshape(-1).view(np.int32), want.view(np.int32))


def test_restatement_matches_live_pillow():
    """Only where Pillow imports: the restatement against Image.resize itself, on the cases' sources and on sizes the golden does not hold."""
    Image = pytest.importorskip("PIL.Image")
    for name, H, W, Ho, Wo in ic.CASES + (("extra_h40w23", 40, 23, 17, 31), ("extra_h2w2", 2, 2, 7, 7)):
        rgba = ic.source(name, H, W)
        for bg in ic.BACKGROUNDS:
            rgb = rgba[:, :, :3]
            if bg == "white":
                pil = Image.fromarray(rgba, "RGBA")
                canvas = Image.new("RGBA", pil.size, "WHITE")
                canvas.paste(pil, (0, 0), pil)
                rgb = np.asarray(canvas.convert("RGB"))
            elif bg == "premasked":
                rgb = rgb * np.uint8(rgba[:, :, 3:] > 0)
            want = np.asarray(Image.fromarray(np.ascontiguousarray(rgb)).resize((Wo, Ho), Image.LANCZOS))
            mask = np.asarray(Image.fromarray((rgba[:, :, 3] > 0).astype(float)).resize((Wo, Ho), Image.NEAREST))
            b, _, m = ic.ingest(rgba, Ho, Wo, bg)
            assert int((b != want).sum()) == 0 and np.array_equal(m[0], mask.astype(np.float32)), (name, bg)

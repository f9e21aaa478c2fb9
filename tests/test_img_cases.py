"""CPU: the image message input's contract and case table (tests/_img_cases.py).  The NumPy restatement of message -> planes equals an
independent per-pixel struct.unpack loop; the descriptor accepts every encoding of the contract and raises for everything the entry
point would refuse; the oracle's correspondence of every case -- on the map state the GPU test starts from -- samples the image's first
and last row, first and last column and its last pixel; the table reaches every k_image_frame variant the launcher can select."""
import numpy as np
import pytest

import _img_cases as ic


def test_the_table_is_what_it_says():
    keys = [ic.case_key(c) for c in ic.CASES]
    assert len(keys) == len(set(keys)) and 40 <= len(keys) <= 80
    for e in range(7):
        mine = [c for c in ic.CASES if c["elem"] == e and (c["H"], c["W"]) == (48, 64)]
        assert {c["n_chan"] for c in mine} == {1, 2, 3, 4}, ic.ELEMS[e]
        assert {c["step_mode"] for c in mine} == set(ic.STEP_MODES), ic.ELEMS[e]
        if ic.SIZES[e] > 1:
            assert {c["big"] for c in mine} == {False, True}, ic.ELEMS[e]
            assert any(c["big"] and c["step_mode"] == "odd" for c in mine) and any(not c["big"] and c["step_mode"] == "odd" for c in mine), ic.ELEMS[e]
    assert {c["enc"] for c in ic.CASES} >= set(ic.NAMED)
    assert {(c["H"], c["W"]) for c in ic.CASES} == {(48, 64), (1, 1), (5, 3)}
    assert {c["C"] for c in ic.CASES} == {66, 98} and sum(c["C"] == 98 for c in ic.CASES) == 1
    for c in ic.CASES:
        tight = c["W"] * c["n_chan"] * ic.SIZES[c["elem"]]
        assert c["step"] >= tight and (c["step"] == tight) == (c["step_mode"] == "tight")
        assert c["step_mode"] != "odd" or c["step"] % 2 == 1
        assert c["step_mode"] != "pad64" or (c["step"] % 64 == 0 and c["step"] > tight)
        assert sum(3 if ch == "rgb" else 1 for ch in c["channels"]) == c["n_chan"] and 1 <= len(c["channels"]) <= 4
        assert "rgb" not in c["channels"] or ic.ELEMS[c["elem"]] in ("8U", "16U")            # colour: values >= 0 only
    assert any(len(set(c["channels"])) < len(c["channels"]) for c in ic.CASES)               # one layer named twice


def test_every_kernel_variant_is_reached():
    from elevation_mapping_cupy_amd.elevation_mapping import IMAGE_ELEM_SIZE
    assert tuple(IMAGE_ELEM_SIZE) == ic.SIZES
    hit = {c["variant"] for c in ic.CASES}
    assert hit == set(range(ic.N_VARIANTS))
    for c in ic.CASES:
        assert c["variant"] == ic.VARIANT_OF_SIZE[IMAGE_ELEM_SIZE[c["elem"]]]
    # the launcher's rule (csrc/emap_launch.h: image_frame_variant) is by element size: 1, 2, 4, 8 bytes and nothing else
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_launch.h")).read()
    assert re.search(r"image_frame_variant\(int esize\) \{ return esize == 1 \? 0 : esize == 2 \? 1 : esize == 4 \? 2 : 3; \}", src)
    kern = open(os.path.join(ROOT, "elevation_mapping_cupy_amd", "csrc", "emap_image_msg.hip")).read()
    assert sorted(set(re.findall(r"k_image_frame<(\d)>\)", kern))) == ["1", "2", "4", "8"]


def test_the_values_make_mistakes_visible():
    for c in ic.CASES:
        v = ic.values(c)
        assert v.shape == (c["H"], c["W"], c["n_chan"])
        e = ic.ELEMS[c["elem"]]
        flat = v.reshape(-1)
        if e in ("16U", "16S", "32S"):
            assert len(np.unique(flat)) == flat.size, ic.case_key(c)
        elif e in ("32F", "64F"):
            fin = flat[np.isfinite(flat)]
            assert len(np.unique(fin)) >= fin.size - flat.size // 5, ic.case_key(c)           # (the rotating specials repeat)
        elif flat.size >= 256:
            assert len(np.unique(flat)) == 256 and (np.diff(flat[:256].astype(np.int32)) != 0).all(), ic.case_key(c)
        if "rgb" in c["channels"]:
            assert (v >= 0).all()
        data = ic.message(c)
        assert data.size == c["H"] * c["step"]
        tight = c["W"] * c["n_chan"] * ic.SIZES[c["elem"]]
        assert (data.reshape(c["H"], c["step"])[:, tight:] == ic.POISON).all()
    big32 = ic.values(next(c for c in ic.CASES if ic.ELEMS[c["elem"]] == "32S" and c["H"] == 48))
    assert (np.abs(big32.astype(np.int64)) > 1 << 24).mean() > 0.9
    assert (big32.astype(np.float32).astype(np.int64) != big32).mean() > 0.5                    # the conversion rounds
    f64 = ic.values(next(c for c in ic.CASES if ic.ELEMS[c["elem"]] == "64F" and c["H"] == 48))
    assert np.isnan(f64).any() and (np.abs(f64[np.isfinite(f64)]) > 3.5e38).any()


@pytest.mark.parametrize("c", ic.CASES, ids=ic.case_key)
def test_the_restatement_equals_a_per_pixel_unpack(c):
    if (c["H"], c["W"]) == (48, 64) and c["step_mode"] == "pad64" and not c["swap"] and c["enc"] not in ic.NAMED:
        c = dict(c, H=6, W=7, step=ic.step_of("pad64", 7 * c["n_chan"] * ic.SIZES[c["elem"]]))      # (the loop is slow: same code, fewer pixels)
    data = ic.message(c)
    a, b = ic.planes(c, data), ic.planes_loop(c, data)
    assert a.shape == b.shape == (c["n_chan"], c["H"], c["W"]) and a.dtype == np.float32
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    same = (ua == ub) | (np.isnan(a) & np.isnan(b))
    assert same.all(), (ic.case_key(c), np.argwhere(~same)[:3])
    v = ic.values(c)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in range(c["n_chan"]):
            ch = 2 - p if c["swap"] and p in (0, 2) else p
            want = v[:, :, ch].astype(np.float32)
            assert ((a[p] == want) | (np.isnan(a[p]) & np.isnan(want))).all(), (ic.case_key(c), p)
    if ic.ELEMS[c["elem"]] == "64F" and c["H"] * c["W"] * c["n_chan"] > 40:
        assert np.isinf(a).any() and np.isnan(a).any() and (a == np.float32(1e-40)).any() and np.float32(1e-40) != 0


def test_the_descriptor_accepts_the_contract_and_refuses_the_rest():
    from elevation_mapping_cupy_amd.elevation_mapping import image_encoding, image_message_descriptor
    for ei, e in enumerate(ic.ELEMS):
        assert image_encoding(e + "C") == (ei, 1, False)
        for n in (1, 2, 3, 4):
            assert image_encoding("%sC%d" % (e, n)) == (ei, n, False)
    for enc, (e, n, swap) in ic.NAMED.items():
        assert image_encoding(enc) == (ic.ELEMS.index(e), n, swap)
    assert [enc for enc, v in ic.NAMED.items() if v[2]] == ["bgr8", "bgra8"]                  # bgr16 / bgra16 pass unswapped, as in the node
    for enc in ic.REFUSED_ENCODINGS:
        with pytest.raises(ValueError):
            image_encoding(enc)
        with pytest.raises(ValueError):
            image_message_descriptor(enc, 4, 4)
    for c in ic.CASES:
        d = image_message_descriptor(c["enc"], c["H"], c["W"], c["step"], c["big"])
        assert (d.height, d.width, d.step, d.elem, d.n_chan, d.is_bigendian, d.swap_rb) == (c["H"], c["W"], c["step"], c["elem"], c["n_chan"], int(c["big"]), int(c["swap"]))
    assert image_message_descriptor("rgb16", 3, 5).step == 30
    bad = [dict(height=0), dict(width=0), dict(height=-1), dict(height=8193), dict(width=8193), dict(step=29), dict(step=0), dict(step=-30),
           dict(height=8192, width=8192, encoding="64FC4"),                # height * step = 2^31
           dict(height=4097, width=4096, encoding="8UC1")]                 # height * width > 2^24
    for change in bad:
        kw = dict(dict(encoding="rgb16", height=3, width=5, step=30), **change)
        with pytest.raises(ValueError):
            image_message_descriptor(kw["encoding"], kw["height"], kw["width"], None if "encoding" in change else kw["step"])
    assert image_message_descriptor("8UC1", 4096, 4096).step == 4096 and image_message_descriptor("rgb8", 8192, 1, 3).n_chan == 3


@pytest.mark.parametrize("key", sorted(ic.POSES))
def test_the_oracle_alone_samples_the_borders_and_the_last_pixel(key):
    C, H, W = key
    assert any((c["C"], c["H"], c["W"]) == key for c in ic.CASES)
    P, m, center = ic.oracle_state(C)
    assert int((m[2] == 1).sum()) > 0.7 * C * C and np.any(center[:2] != 0)
    v, u = ic.sampled_pixels(C, H, W)
    assert v.size >= 100 and v.min() >= 0 and u.min() >= 0 and v.max() <= H - 1 and u.max() <= W - 1
    assert (v == 0).any() and (v == H - 1).any() and (u == 0).any() and (u == W - 1).any()
    assert ((v == H - 1) & (u == W - 1)).any()              # the pixel whose bytes end the message
    assert ((v == 0) & (u == 0)).any()                      # ... and the one that starts it


def test_every_case_has_a_pose_and_its_samples_include_the_special_values():
    for c in ic.CASES:
        assert (c["C"], c["H"], c["W"]) in ic.POSES, ic.case_key(c)
    # the rotating specials of the float types sit on every fifth serial: the sampled pixels of the 48 x 64 pose hit NaN, +-inf and the
    # subnormal in every float case (so the GPU comparison sees them)
    v, u = ic.sampled_pixels(66, 48, 64)
    for c in ic.CASES:
        if ic.ELEMS[c["elem"]] in ("32F", "64F") and (c["H"], c["W"], c["C"]) == (48, 64, 66):
            pl = ic.planes(c, ic.message(c))
            for kind, name, plane in ic.entries(c):
                got = pl[plane][v, u]
                assert np.isnan(got).any() and np.isposinf(got).any() and np.isneginf(got).any() and (got == np.float32(1e-40)).any(), (ic.case_key(c), plane)

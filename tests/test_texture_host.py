"""Texture lookup on the CPU (tests/texture_sets.py): the conditions the texture cards' rays have to meet, the oracle against the real
reference's recorded answers (tests/golden/texture_rays.npz) and, where oracle/_ref is built, against the live reference on other
seeds; getColor restated in numpy against the oracle for every ray; and the host layer's route from a .crtscene and its image files
to the flattened scene's texture table, for every decoder the parser has."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

import texture_sets as ts
from helpers import assert_same_floats, assert_same_hits

_oracle_answers = {}


def fixture_scene(name):
    """the scene made again from its seed; it is the fixture's (blob and rays compared byte for byte)"""
    fx = ts.load_fixture()[name]
    scene = ts.make(name)
    assert ts.blob(scene) == fx["blob"], name + ": the generator's scene is not the fixture's"
    rays, card = ts.rays(scene)
    assert np.array_equal(rays.view(np.uint32), fx["rays"].view(np.uint32)) and np.array_equal(card, fx["card"]), name + ": the rays are not the fixture's"
    return scene, fx


def oracle_answers(oracle, name):
    if name not in _oracle_answers:
        scene, fx = fixture_scene(name)
        _oracle_answers[name] = ts.oracle_answers(oracle, scene, fx["rays"])
    return _oracle_answers[name]


def compare(got, want, what):
    assert_same_floats(got["frame"], want["frame"], what + ": frame")
    assert_same_hits(got["hits"], want["hits"], what + ": hit records")
    for d in ts.DEPTHS:
        assert_same_floats(got["shoot"][d], want["shoot"][d], what + ": shootRay at depth %d" % d)


# ---- 1. the inputs
def test_the_census_of_the_fixture_holds():
    """every class of texture_sets.required_classes has a ray, every texel of the small bitmaps shows in some colour of the reference,
    and nearly every colour on a bitmap card is lit: counted again from the committed answers, and equal to the recorded census"""
    total = {}
    for name in ts.SCENES:
        scene, fx = fixture_scene(name)
        ts.add_census(total, ts.full_census(scene, fx["card"], fx))
    print("census: %s" % json.dumps(total, sort_keys=True, default=list))
    ts.check_census(total)
    recorded = json.loads(str(np.ravel(np.load(ts.GOLDEN)["census"])[0]))
    assert json.loads(json.dumps(total, sort_keys=True, default=list)) == recorded
    assert sum(len(ts.load_fixture()[n]["rays"]) for n in ts.SCENES) >= 3000
    assert os.path.getsize(ts.GOLDEN) <= 190215            # the largest fixture before this one (uvwrap.npz)


def test_bitmaps_are_not_square_and_one_comes_first():
    scene = ts.make("shapes")
    shapes = [t["_pixels"].shape[1::-1] for t in scene["textures"] if t["type"] == "bitmap"]
    assert shapes == ts.SHAPES and shapes[0][0] != shapes[0][1]
    for w, h in shapes:
        px = ts.texels(w, h).reshape(-1, 3)
        assert len({tuple(p) for p in px}) == w * h and px.min() > 0


def test_x86_conversions_of_the_restatement():
    """the rules themselves, on values whose answers the Intel manual gives (cvttss2si: truncation, or the integer indefinite)"""
    f = np.array([0.0, -0.0, 1.9, -1.9, 2147483520.0, 2147483648.0, -2147483648.0, -2147483904.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert ts.x86_int(f).tolist() == [0, 0, 1, -1, 2147483520, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31]
    g = np.array([0.0, 1.9, -1.0, -1.9, 2147483648.0, 4294967296.0, 4294967808.0, 2.0 ** 62, 2.0 ** 63, -2.0 ** 63, -2.0 ** 40 - 2.0 ** 20, np.inf, np.nan], dtype=np.float32)
    assert ts.x86_uint(g).tolist() == [0, 1, 0xFFFFFFFF, 0xFFFFFFFF, 0x80000000, 0, 512, 0, 0, 0, 0xFFF00000, 0, 0]


# ---- 2. the oracle against the reference
@pytest.mark.parametrize("name", ts.SCENES)
def test_oracle_equals_the_fixture(oracle, name):
    compare(oracle_answers(oracle, name), ts.load_fixture()[name], name)


@pytest.mark.parametrize("seed", ts.LIVE_SEEDS)
@pytest.mark.parametrize("name", ts.SCENES)
def test_oracle_equals_the_live_reference(oracle, name, seed):
    if not oracle.reference_available(True):
        pytest.skip("oracle/_ref not built here")
    scene = ts.make(name, seed)
    rays, card = ts.rays(scene, seed)
    want = ts.reference_answers(oracle, scene, rays)
    assert int((want["hits"]["hit"] == 1).sum()) >= 0.95 * len(rays)
    compare(ts.oracle_answers(oracle, scene, rays), want, "%s, seed %d" % (name, seed))


def test_the_fixture_is_what_its_script_writes(oracle):
    if not oracle.reference_available(True):
        pytest.skip("oracle/_ref not built here")
    from golden import make_texture_rays
    with open(ts.GOLDEN, "rb") as f:
        committed = f.read()
    assert make_texture_rays.fixture_bytes() == committed


# ---- 3. getColor in numpy against the oracle
@pytest.mark.parametrize("name", ts.SCENES)
def test_numpy_getcolor_equals_the_reference_and_the_oracle_for_every_ray(oracle, name):
    """For every ray that meets the card it was aimed at, the colour (0 + k0 albedo) + k1 albedo with the restatement's albedo, computed
    from the REFERENCE's recorded hit, is the reference's recorded colour bit for bit -- and so the oracle's --, and on bitmap cards the
    texel that colour is parallel to is the restatement's y * w + x."""
    scene, fx = fixture_scene(name)
    hits, got = fx["hits"], fx["shoot"][ts.DEPTHS[0]]
    assert_same_floats(oracle_answers(oracle, name)["shoot"][ts.DEPTHS[0]], got, name + ": the oracle's colours")
    look = ts.lookup(scene, hits)
    cards = scene["_info"]["cards"]
    aimed = np.array([cards[k]["mesh"] for k in fx["card"]])
    on = (hits["hit"] == 1) & (hits["mesh"] == aimed) & look["textured"]
    assert int(on.sum()) >= 0.9 * sum(c["texture"] is not None for c in cards) / len(cards) * len(hits)
    assert_same_floats(ts.colours(scene, hits[on], look["albedo"][on]), got[on], name + ": colours")
    checked = 0
    for t, tex in enumerate(scene["textures"]):
        rows = np.flatnonzero(on & (look["texture"] == t))
        if tex["type"] != "bitmap" or not len(rows):
            continue
        found = ts.texel_of_colour(tex["_pixels"], got[rows])
        want = look["y"][rows] * tex["_pixels"].shape[1] + look["x"][rows]
        assert np.array_equal(found, want), "%s, %s: %d texels differ" % (name, tex["name"], int((found != want).sum()))
        checked += len(rows)
    assert checked >= 30


# ---- 4. the host layer: .crtscene and image files -> texture table
def texture_table(hs):
    d = hs.desc
    texels = np.ctypeslib.as_array(d.texels, shape=(d.n_texels * 3,)).copy().reshape(-1, 3) if d.n_texels else np.zeros((0, 3), dtype=np.uint8)
    return [d.textures[i] for i in range(d.n_textures)], texels


def same_float(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


@pytest.mark.parametrize("name", ts.GPU_SCENES)
def test_scene_file_route_keeps_every_texture_and_uv(pkg, scenes, name, tmp_path):
    scene = ts.make(name)
    scenes.write_bitmaps(scene, str(tmp_path))
    hs = pkg.Scene(json_text=ts.to_json(scene), folder=str(tmp_path))
    table, texels = texture_table(hs)
    assert len(table) == len(scene["textures"])
    offset = 0
    for rec, t in zip(table, scene["textures"]):
        assert rec.kind == scenes.TEXTURE_KINDS[t["type"]], t["name"]
        if t["type"] == "bitmap":
            h, w = t["_pixels"].shape[:2]
            assert (rec.width, rec.height, rec.texel_offset) == (w, h, offset), (t["name"], rec.width, rec.height, rec.texel_offset, offset)
            assert np.array_equal(texels[offset:offset + w * h], t["_pixels"].reshape(-1, 3)), t["name"] + ": texels in row-major order of the source"
            offset += w * h
        elif t["type"] in ("edges", "checker"):
            scalar = t["edge_width"] if t["type"] == "edges" else t["square_size"]
            assert same_float(rec.scalar, scalar), (t["name"], rec.scalar, scalar)
            a, b = ("inner_color", "edge_color") if t["type"] == "edges" else ("color_A", "color_B")
            assert all(same_float(x, y) for x, y in zip(list(rec.color_a) + list(rec.color_b), list(t[a]) + list(t[b]))), t["name"]
    assert offset == len(texels)
    d = hs.desc
    uvs = np.ctypeslib.as_array(d.vertex_uvs, shape=(d.n_vertices * 3,)).copy()
    want = np.concatenate([o["uvs"].ravel() for o in scene["objects"]])
    assert np.array_equal(uvs.view(np.uint32), want.view(np.uint32)), "vertex UVs, infinities and -0 among them, bit for bit"


def test_what_a_scene_file_cannot_say_is_refused(pkg, scenes):
    """a NaN has no JSON spelling: the parser refuses the text (the blob route keeps such scenes for the oracle and the reference)"""
    scene = ts.make("hostonly")
    text = scenes.to_json(scene)
    assert "nan" in text
    with pytest.raises(pkg.CrtError):
        pkg.Scene(json_text=text)
    with pytest.raises(AssertionError):
        ts.to_json(scene)


def _png(px):
    h, w, c = px.shape
    raw = b"".join(b"\x00" + px[y].tobytes() for y in range(h))
    chunk = lambda tag, body: struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) +
            chunk(b"IEND", b""))


def _bmp(px, top_down=False):
    h, w, c = px.shape
    bgr = px[:, :, [2, 1, 0] + ([3] if c == 4 else [])]
    stride = (w * c + 3) // 4 * 4
    rows = [bgr[y].tobytes() + b"\x00" * (stride - w * c) for y in (range(h) if top_down else range(h - 1, -1, -1))]
    head = struct.pack("<IiiHHIIiiII", 40, w, -h if top_down else h, 1, 8 * c, 0, stride * h, 2835, 2835, 0, 0)
    return b"BM" + struct.pack("<IHHI", 54 + stride * h, 0, 0, 54) + head + b"".join(rows)


def _tga(px, top_down=False):
    h, w, c = px.shape
    bgr = px[:, :, [2, 1, 0] + ([3] if c == 4 else [])]
    body = b"".join(bgr[y].tobytes() for y in (range(h) if top_down else range(h - 1, -1, -1)))
    return struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, w, h, 8 * c, (0x20 if top_down else 0) | (8 if c == 4 else 0)) + body


def _pnm(px, ascii_=False):
    h, w, _ = px.shape
    if ascii_:
        return b"P3\n# a comment\n%d %d\n255\n" % (w, h) + b" ".join(b"%d" % v for v in px.ravel()) + b"\n"
    return b"P6\n%d %d\n255\n" % (w, h) + px.tobytes()


def image_files():
    """(file name, bytes, RGB texels uint8 [h, w, 3]): every decoder at two asymmetric shapes, with 3 and with 4 channels"""
    out = []
    for k, (w, h) in enumerate([(5, 3), (3, 7)]):
        rgb = ts.texels(w, h)
        y, x = np.mgrid[0:h, 0:w]
        rgba = np.concatenate([rgb, (3 + 11 * x + 29 * y).astype(np.uint8)[:, :, None]], axis=2)
        tag = "%dx%d" % (w, h)
        out += [("/p6_%s.ppm" % tag, _pnm(rgb), rgb), ("/p3_%s.ppm" % tag, _pnm(rgb, True), rgb),
                ("/rgb_%s.png" % tag, _png(rgb), rgb), ("/rgba_%s.png" % tag, _png(rgba), rgb),
                ("/rgb_%s.bmp" % tag, _bmp(rgb, top_down=bool(k)), rgb), ("/rgba_%s.bmp" % tag, _bmp(rgba, top_down=not k), rgb),
                ("/rgb_%s.tga" % tag, _tga(rgb, top_down=bool(k)), rgb), ("/rgba_%s.tga" % tag, _tga(rgba, top_down=not k), rgb)]
    return out


def test_every_decoder_keeps_width_height_offset_and_row_order(pkg, scenes, tmp_path):
    """PNG, PNM, BMP and TGA at 5x3 and 3x7 with 3 and 4 channels, all in one scene: each texture's own w, h and offset,
    texels in the row-major order of the source array, a fourth channel dropped.  (One- and two-channel images stay out: the
    reference reads past its buffer for them, Texture.cpp:55-57.)"""
    files = image_files()
    scene = ts.make("hostonly")
    scene["textures"] = [{"name": "img%d" % i, "type": "bitmap", "file_path": path, "_pixels": rgb} for i, (path, _, rgb) in enumerate(files)]
    scene["materials"] = [{"type": "diffuse", "albedo": "img%d" % (i % len(files)), "smooth_shading": False} for i in range(len(scene["materials"]))]
    for path, data, _ in files:
        (tmp_path / path[1:]).write_bytes(data)
    hs = pkg.Scene(json_text=scenes.to_json(scene), folder=str(tmp_path))         # (the table points into the scene: keep it)
    table, texels = texture_table(hs)
    offset = 0
    for rec, (path, _, rgb) in zip(table, files):
        h, w = rgb.shape[:2]
        assert (rec.kind, rec.width, rec.height, rec.texel_offset) == (scenes.TEXTURE_KINDS["bitmap"], w, h, offset), path
        assert np.array_equal(texels[offset:offset + w * h], rgb.reshape(-1, 3)), path
        offset += w * h
    assert offset == len(texels) == sum(r.shape[0] * r.shape[1] for _, _, r in files)

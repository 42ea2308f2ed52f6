"""What the tests of lightmap baking (crt_bake_texels_device, crt_bake_dilate_device, crt_bake_lightmap) share: the rule of include/crt_hip.h
("Lightmap baking"; csrc/bake_rule.h) restated in numpy -- every line one float32 operation, in the header's order, so a float32 numpy
expression rounds it as the -ffp-contract=off build rounds it --, and the small cases it runs on.  numpy only, no GPU.

The scene is the HW12-like room at a low detail with two meshes more: a free-standing quad(nu=2, nv=2) wall whose UVs fill part of the map,
and a hand-made mesh of five triangles: two with identical UVs (the tie), one with zero UV area, one with an infinite UV (a .crtscene
cannot carry a NaN; the rule's host tests put one in), and one whose UVs lie partly outside [0, 1] and whose box is large."""
import ctypes as C

import numpy as np

F32 = np.float32
U32 = np.uint32
NO_OWNER = 0xFFFFFFFF
EMPTY, COVERED, DILATED = 0, 1, 2
MAPS = [(13, 7), (33, 70), (64, 64)]          # (width, height): non-square, no multiples of the 32x8 tile, one narrower than a wave
LARGE_MAP = (96, 64)                          # the hand-made mesh's last triangle has a box of more than 4096 texels here
WAVE_TEXELS = 4096                            # kernel_bake.h: BAKE_WAVE_TEXELS
SCENE_PARAMS = dict(width=64, height=48, detail=0.04, bitmap_size=16)
CASES = {"knot": 5, "sphere": 6, "quad": 9, "hand": 10}   # mesh indices of the scene below
NEIGHBOURS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]
HAND_UVS = [[(0.55, 0.55), (0.95, 0.6), (0.7, 0.95)],      # 0, 1: identical UVs
            [(0.55, 0.55), (0.95, 0.6), (0.7, 0.95)],
            [(0.1, 0.8), (0.2, 0.8), (0.3, 0.8)],          # 2: zero UV area
            [(np.inf, 0.5), (0.6, 0.1), (0.9, 0.3)],       # 3: a non-finite UV
            [(-0.4, -0.3), (1.3, 0.1), (0.1, 0.8)]]        # 4: partly outside [0, 1], large


def hand_mesh(scenes):
    """five separate triangles on planes z = -2.0 - 0.05 k, facing +z"""
    layout = [HAND_UVS[0], HAND_UVS[1], [(0.1, 0.8), (0.2, 0.7), (0.3, 0.8)], [(0.5, 0.5), (0.6, 0.1), (0.9, 0.3)], HAND_UVS[4]]
    verts, uvs, tris = [], [], []
    for k, (lay, uv) in enumerate(zip(layout, HAND_UVS)):
        for (lu, lv), (u, v) in zip(lay, uv):
            verts.append((-1.0 + 2.0 * lu, -0.5 + 1.5 * lv, -2.0 - 0.05 * k))
            uvs.append((u, v, 0.0))
        tris.append((3 * k, 3 * k + 1, 3 * k + 2))
    return scenes._mesh(4, np.array(verts), np.array(tris), np.array(uvs))


def make_scene(scenes):
    scene = scenes.make("hw12", **SCENE_PARAMS)
    assert len(scene["objects"]) == 9
    scene["objects"].append(scenes.quad(4, (0.4, -1.2, -1.5), (1.6, -1.2, -1.9), (1.6, 0.2, -1.9), (0.4, 0.2, -1.5), nu=2, nv=2, uv_scale=(0.75, 0.75)))
    scene["objects"].append(hand_mesh(scenes))
    return scene


def scene_json(scenes, scene):
    """the .crtscene text; an infinite UV is written as 1e999, which the parser reads as inf"""
    import re
    text = scenes.to_json(scene)
    assert "nan" not in text
    return re.sub(r'(?<=[\[,:])(-?)inf(?=[,\]}])', r"\g<1>1e999", text)


def host_scene(pkg, scenes, scene, folder):
    scenes.write_bitmaps(scene, folder)
    return pkg.Scene(json_text=scene_json(scenes, scene), folder=folder)


class MeshData:
    """what the rule reads of one mesh of a flattened scene (pkg.Scene.desc): its global triangle indices, ascending, and the scene's
    triangle_vertices, vertex_uvs and crt_triangle records"""

    def __init__(self, pkg, hs, mesh):
        d = hs.desc
        L = pkg.lib()
        first = 0
        for m in range(mesh + 1):
            nv, nt = C.c_uint32(), C.c_uint32()
            L.crt_host_mesh_sizes(hs._h, m, C.byref(nv), C.byref(nt))
            if m < mesh:
                first += nt.value
        self.mesh = mesh
        self.tris = np.arange(first, first + nt.value, dtype=U32)
        self.tri_verts = np.ctypeslib.as_array(d.triangle_vertices, shape=(d.n_triangles * 3,)).reshape(-1, 3).copy()
        self.uvs = np.ctypeslib.as_array(d.vertex_uvs, shape=(d.n_vertices * 3,)).reshape(-1, 3).copy()
        self.records = np.ctypeslib.as_array(C.cast(d.triangles, C.POINTER(C.c_float)), shape=(d.n_triangles, 16)).copy()

    def uv(self, tri):
        """float32 [6]: a.x, a.y, b.x, b.y, c.x, c.y"""
        return self.uvs[self.tri_verts[tri], :2].reshape(6).astype(F32)


# ------------------------------------------------------------------------------------------------------------------------ the rule
def centres(width, height, rows, cols):
    cx = cols.astype(F32) + F32(0.5)
    cy = rows.astype(F32) + F32(0.5)
    x = cx / F32(width)
    y = cy / F32(height)
    return x, F32(1.0) - y


def area(uv):
    ax, ay, bx, by, cx, cy = uv
    e1x, e1y, e2x, e2y = bx - ax, by - ay, cx - ax, cy - ay
    p, q = e1x * e2y, e1y * e2x
    return p - q


def usable(a):
    with np.errstate(invalid="ignore"):
        return bool((a - a) == 0 and a != 0)


def box(uv, width, height):
    """(col0, col1, row0, row1), both ends inclusive, of a triangle whose area is usable"""
    ax, ay, bx, by, cx, cy = uv
    umin, umax = min(ax, bx, cx), max(ax, bx, cx)
    vmin, vmax = min(ay, by, cy), max(ay, by, cy)
    fw, fh = F32(width), F32(height)
    clamp = lambda f, hi: F32(0.0) if f < 0 else (hi if f > hi else f)
    with np.errstate(over="ignore"):
        f0, f1 = clamp(umin * fw, fw), clamp(umax * fw, fw)
        g0, g1 = clamp((F32(1.0) - vmax) * fh, fh), clamp((F32(1.0) - vmin) * fh, fh)
    return max(int(f0) - 1, 0), min(int(f1) + 1, width - 1), max(int(g0) - 1, 0), min(int(g1) + 1, height - 1)


def covers(uv, a, qx, qy):
    """-> (covered bool, e1, e2) for arrays of centres"""
    ax, ay, bx, by, cx, cy = uv
    e1x, e1y, e2x, e2y = bx - ax, by - ay, cx - ax, cy - ay
    dx, dy = qx - ax, qy - ay
    f1 = dx * e2y - dy * e2x
    f2 = e1x * dy - e1y * dx
    bqx, bqy, cqx, cqy = bx - qx, by - qy, cx - qx, cy - qy
    f0 = bqx * cqy - bqy * cqx
    inside = ((f0 >= 0) & (f1 >= 0) & (f2 >= 0)) if a > 0 else ((f0 <= 0) & (f1 <= 0) & (f2 <= 0))
    return inside, f1, f2


def owners(md, width, height, tally=None, uv_of=None):
    """the owner plane uint32 [H, W]: the covering triangle with the lowest index, NO_OWNER where none covers.  tally: boxes walked by a
    wave / listed as large."""
    uv_of = uv_of or md.uv
    own = np.full((height, width), NO_OWNER, dtype=U32)
    for tri in md.tris:                     # ascending: the first to cover a texel is its owner
        uv = uv_of(tri)
        with np.errstate(invalid="ignore", over="ignore"):
            a = area(uv)
        if not usable(a):
            continue
        c0, c1, r0, r1 = box(uv, width, height)
        if c0 > c1 or r0 > r1:
            continue
        if tally is not None:
            tally["large" if (c1 - c0 + 1) * (r1 - r0 + 1) > WAVE_TEXELS else "wave"] += 1
        rows, cols = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing="ij")
        qx, qy = centres(width, height, rows, cols)
        with np.errstate(invalid="ignore", over="ignore"):
            inside, _, _ = covers(uv, a, qx, qy)
        sub = own[r0:r1 + 1, c0:c1 + 1]
        sub[inside & (sub == NO_OWNER)] = tri
    return own


TEXEL_DTYPE = np.dtype([("point", F32, 3), ("u", F32), ("normal", F32, 3), ("v", F32), ("triangle", U32), ("mesh", U32), ("status", U32),
                        ("pad", U32)])


def texels(md, width, height, probe_offset, own=None, uv_of=None):
    """-> (records TEXEL_DTYPE [H, W], probe rays float32 [H, W, 6] (0 where EMPTY), status uint8 [H, W])"""
    uv_of = uv_of or md.uv
    own = owners(md, width, height, uv_of=uv_of) if own is None else own
    rec = np.zeros((height, width), dtype=TEXEL_DTYPE)
    rays = np.zeros((height, width, 6), dtype=F32)
    rec["triangle"] = own
    rec["mesh"] = md.mesh
    off = F32(probe_offset)
    for tri in np.unique(own[own != NO_OWNER]):
        rows, cols = np.nonzero(own == tri)
        uv = uv_of(tri)
        a = area(uv)
        qx, qy = centres(width, height, rows, cols)
        _, e1, e2 = covers(uv, a, qx, qy)
        u, v = e1 / a, e2 / a
        w = (F32(1.0) - u) - v
        T = md.records[tri]
        v0, v1, v2, n = T[0:3], T[4:7], T[8:11], T[[3, 7, 11]]
        point = np.stack([(v0[k] * w + v1[k] * u) + v2[k] * v for k in range(3)], axis=1).astype(F32)
        rec["point"][rows, cols] = point
        rec["u"][rows, cols] = u
        rec["v"][rows, cols] = v
        rec["normal"][rows, cols] = n
        rec["status"][rows, cols] = COVERED
        rays[rows, cols, 0:3] = point + (n * off)[None, :]
        rays[rows, cols, 3:6] = -n
    return rec, rays, rec["status"].astype(np.uint8)


def fmix32(h):
    h = h.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(U32)


def gi_mix(a, b):
    a, b = np.asarray(a, dtype=U32), np.asarray(b, dtype=U32)
    t = ((b ^ U32(0x7F4A7C15)).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return fmix32(((fmix32(a ^ U32(0x9E3779B9)).astype(np.uint64) + t) & np.uint64(0xFFFFFFFF)).astype(U32))


def keys(gi_seed, p, s):
    """the key of sample s of the texels p (row-major indices)"""
    return gi_mix(gi_mix(np.full(np.shape(p), gi_seed, dtype=U32), p), np.full(np.shape(p), s, dtype=U32))


def fold(colours):
    """the left fold of the samples' colours [n_samples, n, 3] -> the mean [n, 3]"""
    total = None
    for s, c in enumerate(colours):
        c = np.asarray(c, dtype=F32)
        total = (F32(0.0) + c) if s == 0 else (total + c)
    return total * (F32(1.0) / F32(len(colours)))


def dilate(rgb, status, passes):
    """-> (rgb, status) after min(passes, max(W, H)) passes"""
    rgb, status = rgb.copy(), status.copy()
    height, width = status.shape
    for _ in range(min(int(passes), max(width, height))):
        src_rgb, src_status = rgb.copy(), status.copy()
        todo = src_status == EMPTY
        for dr, dc in NEIGHBOURS:
            rows, cols = np.nonzero(todo)
            r, c = rows + dr, cols + dc
            ok = (r >= 0) & (r < height) & (c >= 0) & (c < width)
            ok[ok] &= src_status[r[ok], c[ok]] != EMPTY
            rgb[rows[ok], cols[ok]] = src_rgb[r[ok], c[ok]]
            status[rows[ok], cols[ok]] = DILATED
            todo[rows[ok], cols[ok]] = False
    return rgb, status


def lightmap(colours, rec_status, passes):
    """the map of a bake: colours float32 [covered, 3] in row-major order of the covered texels, EMPTY texels 0, then the dilation"""
    rgb = np.zeros(rec_status.shape + (3,), dtype=F32)
    rgb[rec_status == COVERED] = colours
    return dilate(rgb, rec_status, passes)


def same_records(got, want, what):
    assert got.shape == want.shape, what
    for field in TEXEL_DTYPE.names:
        g, w = np.ascontiguousarray(got[field]), np.ascontiguousarray(want[field])
        bad = np.argwhere(g.view(U32) != w.view(U32))
        assert bad.size == 0, "%s: %s differs at %d places, first %s: got %r want %r" % (what, field, len(bad), bad[0].tolist(), got[tuple(bad[0][:2])],
                                                                                         want[tuple(bad[0][:2])])


# ------------------------------------------------------------------------------------------------------------------------ the probes
def probe_rays(md, width, height, probe_offset=1e-3):
    """the covered texels of a map in row-major order: (texel indices uint32 [n], probe rays float32 [n, 6], records [n])"""
    rec, rays, status = texels(md, width, height, probe_offset)
    keep = status.ravel() == COVERED
    return np.flatnonzero(keep).astype(U32), rays.reshape(-1, 6)[keep], rec.reshape(-1)[keep]


def oracle_shoot(o, rays, max_depth=5):
    """OracleScene.shoot of every ray as a REFLECTION ray -> float32 [n, 3]"""
    return np.array([o.shoot(r[:3], r[3:], 2, 0, max_depth) for r in rays], dtype=F32).reshape(-1, 3)


def oracle_self_hits(o, md, rays, rec):
    """the probes whose closest hit (OracleScene.trace, whose triangle index is the mesh's own) is the texel's owner"""
    count = 0
    for r, t in zip(rays, rec):
        hit, h = o.trace(r[:3], r[3:], 2)
        count += bool(hit) and int(h[9]) == md.mesh and int(md.tris[0]) + int(h[10]) == int(t["triangle"])
    return count

"""Pure-torch restatement of csrc_recon/meshtangent.hip (test oracle), fp64 by default; with dtype=torch.float32 what that run loses against
the fp64 one is the cost of the number format (the bar idiom of tests/mesh_render_ref.py).  Written from the statements of
include/v3d_recon.h "Tangent space and GLB".  Also a GLB parser written from the glTF 2.0 specification, independent of
v3d_amd.recon.mesh_gltf.read_glb.

Everything is fed GIVEN inputs (normals, frames, a view's face_id / pix_w / pix_tex / pix_tw): no earlier stage is decided again here."""
from __future__ import annotations

import functools
import io
import json
import math
import struct

import numpy as np
import torch

import mesh_bake_ref as B
import mesh_clean_ref as C
import mesh_refine_ref as RF
import mesh_render_ref as M
import mesh_texture_ref as TX

F64, F32 = torch.float64, torch.float32
LEN2_EPS = 1e-20
DET_EPS = 1e-12
EXCLUDE_MAX = M.EXCLUDE_MAX          # at most 2 % of a case may be left out
W_SIGN = -1.0                        # the header's w (the CPU test derives it from the definition)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _unit(x):
    """(x / |x| where |x|^2 > 1e-20 else x, which rows had a direction, |x|^2)"""
    len2 = _dot(x, x)
    ok = len2 > LEN2_EPS
    return torch.where(ok[..., None], x / torch.sqrt(torch.where(ok, len2, torch.ones_like(len2)))[..., None], x), ok, len2


def near(len2, eps=LEN2_EPS):
    """a squared length (or |det|) within a factor 2 of its threshold: the only reason to leave an element out of a comparison"""
    return (len2 >= eps / 2) & (len2 <= eps * 2)


def _up(like):
    z = torch.zeros_like(like)
    z[..., 2] = 1
    return z


# ---- 1. corner frames -------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def corner_frames(verts, faces, normals, dtype=F64):
    """dict(cn [3F, 3], ct [3F, 4], valid [3F] (the face's indices are vertices), keep [3F] (no length within a factor 2 of the 1e-20 rule),
    fallback [3F] (the tangent came from the basis of N))"""
    V, F = verts.shape[0], faces.shape[0]
    f = faces.long()
    ok = ((f >= 0) & (f < V)).all(1)
    fz = torch.where(ok[:, None], f, torch.zeros_like(f))
    v, n = verts.to(dtype), normals.to(dtype)
    s = torch.where((torch.arange(F) & 1) == 1, -1.0, 1.0).to(dtype)
    se1 = (s[:, None] * (v[fz[:, 1]] - v[fz[:, 0]])).repeat_interleave(3, 0)
    N, has_n, n2 = _unit(n[fz.reshape(-1)])
    N = torch.where(has_n[:, None], N, _up(N))
    d = _dot(N, se1)
    T, has_t, t2 = _unit(se1 - N * d[:, None])
    q = torch.where(torch.signbit(N[:, 2]), -1.0, 1.0).to(dtype)          # copysign(1, N.z)
    a = -1.0 / (q + N[:, 2])
    b = N[:, 0] * N[:, 1] * a
    t1 = torch.stack([1 + q * N[:, 0] * N[:, 0] * a, q * b, -q * N[:, 0]], 1)
    T = torch.where(has_t[:, None], T, t1)
    valid = ok.repeat_interleave(3)
    cn = torch.where(valid[:, None], N, _up(N))
    ct = torch.cat([torch.where(valid[:, None], T, torch.tensor([1.0, 0.0, 0.0], dtype=dtype).expand_as(T)), torch.full((3 * F, 1), W_SIGN, dtype=dtype)], 1)
    return dict(cn=cn, ct=ct, valid=valid, keep=~valid | ~(near(n2) | near(t2)), fallback=valid & ~has_t)


def derived_w(verts, faces, cn, ct):
    """[3F]: sign(cross(N, T) . (-dP/dv)) in fp64 from the definition: glTF's bitangent w cross(N, T) points along DECREASING v, and in the
    atlas dP/dv = s e2 / L"""
    v, f = verts.double(), faces.long()
    s = torch.where((torch.arange(f.shape[0]) & 1) == 1, -1.0, 1.0).double()
    dPdv = (s[:, None] * (v[f[:, 2]] - v[f[:, 0]])).repeat_interleave(3, 0)
    return torch.sign(_dot(_cross(cn.double(), ct.double()[:, :3]), -dPdv))


# ---- 2. the frame at a point, decode, encode --------------------------------------------------------------------------------------------------
def frame_at(cn, ct, f, b, dtype=F64):
    """(vN, vT, vB) [n, 3] at barycentrics b [n, 3] of faces f [n] from the corner rows"""
    cn, ct, b = cn.to(dtype), ct.to(dtype), b.to(dtype)
    rows = 3 * f[:, None] + torch.arange(3)[None]
    mix = lambda a: b[:, 0:1] * a[rows[:, 0]] + b[:, 1:2] * a[rows[:, 1]] + b[:, 2:3] * a[rows[:, 2]]  # noqa: E731
    vN, vT = mix(cn), mix(ct[:, :3])
    return vN, vT, _cross(vN, vT) * ct[rows[:, 0], 3:4]


def decode(fr, c):
    """(n [n, 3], keep [n]): c.x vT + c.y vB + c.z vN normalised; normalise(vN), then (0, 0, 1), on a vanishing length"""
    vN, vT, vB = fr
    raw = c[:, 0:1] * vT + c[:, 1:2] * vB + c[:, 2:3] * vN
    n, ok, l2 = _unit(raw)
    nn, ok_n, n2 = _unit(vN)
    back = torch.where(ok_n[:, None], nn, _up(nn))
    return torch.where(ok[:, None], n, back), ~(near(l2) | (~ok & near(n2)))


def encode(fr, m):
    """(c [n, 3], keep [n], det [n])"""
    vN, vT, vB = fr
    bn, nt, tb = _cross(vB, vN), _cross(vN, vT), _cross(vT, vB)
    det = _dot(vT, bn)
    good = torch.isfinite(det) & (det.abs() > DET_EPS)
    safe = torch.where(good, det, torch.ones_like(det))
    c = torch.stack([_dot(m, bn) / safe, _dot(m, nt) / safe, _dot(m, tb) / safe], 1)
    cu, ok, c2 = _unit(c)
    ok = ok & torch.isfinite(c2) & good
    return torch.where(ok[:, None], cu, _up(cu)), ~(near(det.abs(), DET_EPS) | (good & near(c2))), det


def _texels(faces, num_verts, R, dtype):
    F = faces.shape[0]
    S, _ = TX.layout(F, R)
    owner, i, j = TX.texel_cells(F, R)
    tri = faces.long()[owner.clamp_min(0)]
    live = (owner >= 0) & ((tri >= 0) & (tri < num_verts)).all(1)
    L = torch.tensor(float(S - 3), dtype=dtype)
    b1 = (i.to(dtype) / L).clamp(0, 1)
    b2 = torch.minimum((j.to(dtype) / L).clamp_min(0), 1 - b1)
    return owner, live, torch.stack([1 - b1 - b2, b1, b2], 1)


@torch.no_grad()
def convert_map(faces, num_verts, cn, ct, source, R, encode_it, dtype=F64):
    """dict(owner [R*R], map [R*R, 3], live [R*R] (owned by a face whose indices are vertices), keep [R*R], det [R*R] (encode only, else 0))"""
    owner, live, b = _texels(faces, num_verts, R, dtype)
    fr = frame_at(cn, ct, owner.clamp_min(0), b, dtype)
    src = source.to(dtype)
    if encode_it:
        out, keep, det = encode(fr, src)
    else:
        (out, keep), det = decode(fr, src), torch.zeros(R * R, dtype=dtype)
    return dict(owner=owner, map=torch.where(live[:, None], out, _up(out)), live=live, keep=keep | ~live, det=det)


# ---- 3. the lit shade -------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def shade_lit(face_id, pix_w, pix_tex, pix_tw, F, cn, ct, tangent_map, albedo, ao_map, R, light_dirs, light_intensity, ambient, bg, dtype=F64):
    """dict(image [3, H, W], normals [3, H, W], covered [H, W], keep [H, W])"""
    H, W = face_id.shape
    fid = face_id.long().reshape(-1)
    w = pix_w.to(dtype).reshape(-1, 3)
    s = (w[:, 0] + w[:, 1]) + w[:, 2]
    pt = pix_tex.long().reshape(-1, 4)
    cov = (fid >= 0) & (fid < F) & (s > 0) & ((pt >= 0) & (pt < R * R)).all(1)
    s = torch.where(cov, s, torch.ones_like(s))
    idx = pt.clamp(0, R * R - 1)
    q = pix_tw.to(dtype).reshape(-1, 4)
    fr = frame_at(cn, ct, fid.clamp(0, F - 1), w / s[:, None], dtype)
    tap = lambda T: q[:, 0:1] * T[idx[:, 0]] + q[:, 1:2] * T[idx[:, 1]] + q[:, 2:3] * T[idx[:, 2]] + q[:, 3:4] * T[idx[:, 3]]  # noqa: E731
    c = tap(tangent_map.to(dtype)) if tangent_map is not None else _up(torch.zeros(fid.shape[0], 3, dtype=dtype))
    n, keep = decode(fr, c)
    light = torch.full((fid.shape[0],), float(ambient), dtype=dtype)
    if ao_map is not None:
        light = light * tap(ao_map.to(dtype)[:, None])[:, 0]
    for d, i in zip(light_dirs, light_intensity):
        light = light + float(np.float32(i)) * _dot(n, torch.as_tensor(np.asarray(d, dtype=np.float32)).to(dtype)[None]).clamp_min(0)
    img = tap(albedo.to(dtype)) * light[:, None]
    bgt = torch.as_tensor(bg, dtype=dtype).reshape(1, 3)
    return dict(image=torch.where(cov[:, None], img, bgt.expand_as(img)).t().reshape(3, H, W),
                normals=torch.where(cov[:, None], n, torch.zeros_like(n)).t().reshape(3, H, W), covered=cov.reshape(H, W),
                keep=(keep | ~cov).reshape(H, W))


# ---- 4. a GLB parser from the specification ---------------------------------------------------------------------------------------------------
GLB_MAGIC, CHUNK_JSON, CHUNK_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


def parse_glb(raw: bytes) -> dict:
    """Checks the container (glTF 2.0 section 4.4: 12-byte header; chunks of length, type, data, each 4-byte aligned; JSON padded with
    spaces, BIN with zeros) and returns dict(json, bin, json_pad, bin_pad: the padding bytes)."""
    assert len(raw) >= 20 and len(raw) % 4 == 0
    magic, version, total = struct.unpack_from("<III", raw, 0)
    assert magic == GLB_MAGIC and raw[:4] == b"glTF" and version == 2 and total == len(raw)
    n, kind = struct.unpack_from("<II", raw, 12)
    assert kind == CHUNK_JSON and n % 4 == 0 and 20 + n <= len(raw)
    text = raw[20:20 + n]
    body = text.rstrip(b" ")
    gltf = json.loads(body.decode("utf-8"))
    at, blob, bin_pad = 20 + n, b"", b""
    if at < len(raw):
        m, kind = struct.unpack_from("<II", raw, at)
        assert kind == CHUNK_BIN and m % 4 == 0 and at + 8 + m == len(raw)
        blob = raw[at + 8:]
        want = gltf["buffers"][0]["byteLength"]
        assert len(gltf["buffers"]) == 1 and "uri" not in gltf["buffers"][0] and want <= m < want + 4
        bin_pad = blob[want:]
    else:
        assert "buffers" not in gltf
    return dict(json=gltf, bin=blob, json_pad=text[len(body):], bin_pad=bin_pad)


def glb_accessor(g: dict, index: int) -> np.ndarray:
    a = g["json"]["accessors"][index]
    bv = g["json"]["bufferViews"][a["bufferView"]]
    assert a["componentType"] == 5126 and "byteStride" not in bv and "sparse" not in a
    k = COMPONENTS[a["type"]]
    start = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
    assert start + 4 * k * a["count"] <= bv.get("byteOffset", 0) + bv["byteLength"]
    return np.frombuffer(g["bin"], dtype="<f4", count=k * a["count"], offset=start).reshape(a["count"], k)


def glb_image(g: dict, texture_index: int) -> np.ndarray:
    """the decoded pixels [R, R, channels] of a texture's PNG"""
    from PIL import Image
    t = g["json"]["textures"][texture_index]
    im = g["json"]["images"][t["source"]]
    assert im["mimeType"] == "image/png" and "uri" not in im
    bv = g["json"]["bufferViews"][im["bufferView"]]
    data = g["bin"][bv.get("byteOffset", 0):bv.get("byteOffset", 0) + bv["byteLength"]]
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    return np.asarray(Image.open(io.BytesIO(data)))


# ---- 5. scenes --------------------------------------------------------------------------------------------------------------------------------
def fallback_face():
    """(verts, faces, normals): one face whose e1 = (0, 0, 0.5) is parallel to two of its corner normals, exactly in every format: corner 0
    takes the basis of N = (0, 0, 1), corner 1 that of N = (0, 0, -1) (the other branch of the copysign), corner 2 has a tangent of its own"""
    v = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 0.5], [1.0, 0.0, 0.0]])
    n = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -2.0], [0.6, 0.0, 0.8]])
    return v, torch.tensor([[0, 1, 2]]), n


FRAME_CASES = ("sphere", "first1", "first2", "first257", "degenerate", "fallback")


@functools.lru_cache(maxsize=None)
def frame_case(name):
    """(verts, faces, normals float32 GIVEN, scene): `scene` names the case whose float32 figure holds this one (a prefix of the sphere is held
    to the sphere's: 3 corners cannot measure a format)"""
    if name == "fallback":
        return fallback_face() + ("fallback",)
    if name == "degenerate":
        v, f = B.degenerate_mesh()
        return v, f, C.normals(v, f[:320]).float(), "degenerate"
    v, f, _ = M.mesh_scene("sphere", 1)
    n = C.normals(v, f).float()
    return (v, f, n, "sphere") if name == "sphere" else (v, f[:int(name[5:])], n, "sphere")


@functools.lru_cache(maxsize=None)
def frame_restatements(name):
    v, f, n, _ = frame_case(name)
    return corner_frames(v, f, n), corner_frames(v, f, n, F32)


def frame_errors(cn, ct, r64, rows=None):
    rows = r64["keep"] if rows is None else rows & r64["keep"]
    if not bool(rows.any()):
        return 0.0, 0.0
    return float((cn.double() - r64["cn"])[rows].abs().max()), float((ct.double() - r64["ct"])[rows].abs().max())


MAP_SIZES = B.BAKE_SIZES             # 64: S = 4 at 320 faces, the smallest cell; 100: ragged (texels outside g S)
ROTATION_AXIS, ROTATION_ANGLE = (0.3, -0.5, 0.8), 1.1


def rotation():
    """a fixed rotation about no axis of the frame, [3, 3] fp64 (column vectors: x' = Q x)"""
    a = torch.tensor(ROTATION_AXIS, dtype=F64)
    a = a / a.norm()
    K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=F64)
    return torch.eye(3, dtype=F64) + math.sin(ROTATION_ANGLE) * K + (1 - math.cos(ROTATION_ANGLE)) * (K @ K)


def rotated(x):
    """rows of x rotated, rounded to float32: the moved mesh as the kernels get it"""
    return (x.double() @ rotation().t()).float()


def low_mesh():
    """the 320-face icosphere of mesh_bake_ref.bake_scene("nested") and its restated vertex normals (float32)"""
    lv, lf = B.bake_scene("nested")[:2]
    return lv, lf, C.normals(lv, lf).float()


@functools.lru_cache(maxsize=None)
def restated_object_map(R):
    """the bumped sphere's normals baked onto the icosphere by the fp64 restatement, as float32 [R*R, 3]"""
    lv, lf, hv, hf, md = B.bake_scene("nested")
    return B.bake(lv, lf, C.normals(lv, lf).float(), hv, hf, C.normals(hv, hf).float(), R, md)["normal"].float()


def constant_map(R):
    return torch.tensor([0.0, 0.0, 1.0]).expand(R * R, 3).contiguous()


def random_maps(R, seed=4):
    """(albedo [R*R, 3] in 0 .. 1, tangent map [R*R, 3] unit with z > 0, occlusion [R*R] in 0 .. 1)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(R * R, 3, generator=g)
    t[:, 2] = t[:, 2].abs() + 1.0
    return torch.rand(R * R, 3, generator=g), torch.nn.functional.normalize(t, dim=1), torch.rand(R * R, generator=g)


LIT_R = 100
LIT_VIEWS = (("sphere", 1, 64, 64, 0, True), ("sphere", 1, 56, 40, 1, True))
LIT_K = (0, 1, 4)
LIGHTS = (((0.3, -0.5, 0.8), 0.9), ((-0.7, 0.2, 0.1), 0.4), ((0.0, 1.0, 0.0), 0.25), ((0.5, 0.5, -0.7), 0.6))
LIT_AMBIENT = 0.2
LIT_BG = [0.25, 0.5, 0.75]


def lights(K):
    d = np.asarray([x[0] for x in LIGHTS[:K]], dtype=np.float64).reshape(K, 3)
    return [(tuple((row / np.linalg.norm(row)).tolist()), i) for row, (_, i) in zip(d, LIGHTS[:K])]


def light_arrays(K):
    ls = lights(K)
    return [np.asarray(d, dtype=np.float32) for d, _ in ls], [np.float32(i) for _, i in ls]


@functools.lru_cache(maxsize=None)
def lit_view_restatement(view):
    """One lit view wholly on the restatements: dict(face_id, pix_w float32, pix_tex, pix_tw float32, cn, ct float32)"""
    v, f, _, face_id, pw = TX.case_restatement(view)
    pt = TX.pixel_texels(face_id, pw, f.shape[0], LIT_R, F32)
    fr = corner_frames(v, f, C.normals(v, f).float(), F32)
    return dict(verts=v, faces=f, face_id=face_id, pix_w=pw, pix_tex=pt["pix_tex"], pix_tw=pt["pix_tw"].float(), cn=fr["cn"].float(), ct=fr["ct"].float())


# ---- 6. the end-to-end scene (mesh_bake_ref.E2E) ------------------------------------------------------------------------------------------------
@torch.no_grad()
def fidelity_tangent(low_verts, low_faces, low_normals, tangent_map, high_verts, high_faces, high_normals, cameras, dtype=F64):
    """mesh_bake_ref.fidelity's `after` through the tangent map: the mean over the views of the mean angle in degrees between the high mesh's
    rasterized vertex normals and the normals shade_lit decodes per pixel (world space: the angle does not depend on the frame)"""
    R_ = math.isqrt(tangent_map.shape[0])
    fr = corner_frames(low_verts, low_faces, low_normals, dtype)
    bg, after = [0.5, 0.5, 0.5], []
    for cam in cameras:
        W, H = int(cam.width), int(cam.height)
        ph = M.project(high_verts, cam, 8, F32)
        rh = M.rasterize(ph["pix_q"], ph["zv"], high_faces, (high_normals.float() + 1) * 0.5, W, H, bg, cull=True)
        pl = M.project(low_verts, cam, 8, F32)
        rl = M.rasterize(pl["pix_q"], pl["zv"], low_faces, (low_normals.float() + 1) * 0.5, W, H, bg, cull=True)
        _, pw = RF.pixel_weights(pl["pix_q"], pl["zv"], low_faces, rl["face_id"], 8, F32)
        pt = TX.pixel_texels(rl["face_id"], pw, low_faces.shape[0], R_, dtype)
        lit = shade_lit(rl["face_id"], pw, pt["pix_tex"], pt["pix_tw"], low_faces.shape[0], fr["cn"], fr["ct"], tangent_map,
                        torch.zeros(R_ * R_, 3), None, R_, [], [], 0.0, [0.0, 0.0, 0.0], dtype)
        both = (rh["face_id"] >= 0) & (rl["face_id"] >= 0)
        nh = B._unit_image(rh["image"].to(dtype))
        after.append(float(torch.rad2deg(torch.acos((lit["normals"] * nh).sum(0)[both].double().clamp(-1, 1))).mean()))
    return float(np.mean(after))


@functools.lru_cache(maxsize=None)
def e2e_restatement():
    """dict(before (a), object (b), tangent (c), tangent32: (c) with the conversion and the shade in float32) in degrees, on the end-to-end
    scene of mesh_bake_ref wholly on the restatements"""
    sc = B.e2e_cpu()
    (hv, hf, hn), (lv, lf, ln) = sc["high"], sc["low"]
    Rr = B.E2E["tex_size"]
    omap = B.bake(lv, lf, ln, hv, hf, hn, Rr, sc["max_dist"])["normal"]
    before, obj = B.fidelity(lv, lf, ln, omap, hv, hf, hn, sc["cams"])
    out = dict(before=before, object=obj)
    for key, dt in (("tangent", F64), ("tangent32", F32)):
        fr = corner_frames(lv, lf, ln, dt)
        tm = convert_map(lf, lv.shape[0], fr["cn"], fr["ct"], omap, Rr, True, dt)["map"]
        out[key] = fidelity_tangent(lv, lf, ln, tm, hv, hf, hn, sc["cams"], dt)
    return out

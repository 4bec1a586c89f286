"""The mesh texture of libv3d_recon.so (csrc_recon/meshtex.hip, v3d_amd/recon/mesh_texture.py, scripts/pub/texture_mesh.py) without a GPU:
header, ctypes table and exports agree, bad arguments are refused before any launch, the atlas of the header holds what it promises (charts
inside the texture, disjoint ownership, no bilinear weight on a foreign texel), the torch restatement (tests/mesh_texture_ref.py) is honest
(its transpose is autograd's, its loop lowers the loss), the OBJ / MTL / PNG round trip, the script's options, and the premises of the
cases of tests/test_mesh_texture_gpu.py on the restatement alone."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import gs_dense_ref as D
import mesh_refine_ref as RF
import mesh_render_ref as M
import mesh_texture_ref as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEX_ENTRIES = {"v3d_recon_tex_face_uvs", "v3d_recon_tex_bake_vertex_colors", "v3d_recon_tex_pixel_texels", "v3d_recon_tex_shade",
               "v3d_recon_tex_texel_records", "v3d_recon_tex_shade_bwd"}


@pytest.fixture(scope="module")
def lib():
    from v3d_amd.build import build_recon
    from v3d_amd.recon import geometry
    build_recon(verbose=False)
    return geometry.load_library()


def test_header_signatures_and_exports_agree(lib):
    from v3d_amd.recon import geometry
    hdr = open(os.path.join(ROOT, "include", "v3d_recon.h")).read()
    declared = set(re.findall(r"\b(v3d_recon_[a-z_0-9]+)\s*\(", hdr))
    assert TEX_ENTRIES <= declared and TEX_ENTRIES <= set(geometry.SIGNATURES)
    for name in TEX_ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        proto = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(proto.split(",")) == len(geometry.SIGNATURES[name][1]), f"{name}: the ctypes row and the prototype differ in length"
    assert lib.v3d_recon_abi_version() == geometry.ABI_VERSION == 1          # the new entries are additive
    assert "Mesh texture" in hdr and "THE ATLAS" in hdr and os.path.exists(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshtex.hip"))
    src = open(os.path.join(ROOT, "v3d_amd", "csrc_recon", "meshtex.hip")).read()
    assert "atomic" not in src.replace("No atomics", "")


def test_bad_arguments_are_refused_before_any_launch(lib):
    # (no GPU here: an entry that reached its launch would fail differently, or crash; `p` is never dereferenced by the host code)
    p = 0x1000
    err = lambda: lib.v3d_recon_last_error().decode()  # noqa: E731

    def calls(fn, order, **defaults):
        return lambda **kw: fn(*[kw.get(k, defaults[k]) for k in order])

    def atlas_refusals(call, name):
        assert call(F=0) == -1 and name in err() and "positive" in err()
        assert call(R=0) == -1 and "tex_size 0" in err() and "4096" in err()
        assert call(R=4097) == -1 and "tex_size 4097" in err()
        assert call(F=320, R=51) == -1 and "texture too small for 320 faces" in err()        # g = 13, S = 3
        assert call(F=2_000_000_000, R=4096) == -1 and "texture too small" in err()

    uv = calls(lib.v3d_recon_tex_face_uvs, ("F", "R", "vt", "stream"), F=320, R=64, vt=p, stream=None)
    assert uv(vt=None) == -1 and "v3d_recon_tex_face_uvs" in err() and "null" in err()
    atlas_refusals(uv, "v3d_recon_tex_face_uvs")
    bk = calls(lib.v3d_recon_tex_bake_vertex_colors, ("faces", "F", "colors", "V", "R", "fill", "owner", "texture", "stream"),
               faces=p, F=320, colors=p, V=162, R=64, fill=0.5, owner=p, texture=p, stream=None)
    for k in ("faces", "colors", "owner", "texture"):
        assert bk(**{k: None}) == -1 and "v3d_recon_tex_bake_vertex_colors" in err() and "null" in err(), k
    assert bk(V=0) == -1 and "num_verts" in err()
    atlas_refusals(bk, "v3d_recon_tex_bake_vertex_colors")
    pt = calls(lib.v3d_recon_tex_pixel_texels, ("face_id", "pix_w", "F", "R", "W", "H", "pix_tex", "pix_tw", "stream"),
               face_id=p, pix_w=p, F=320, R=64, W=32, H=32, pix_tex=p, pix_tw=p, stream=None)
    for k in ("face_id", "pix_w", "pix_tex", "pix_tw"):
        assert pt(**{k: None}) == -1 and "v3d_recon_tex_pixel_texels" in err() and "null" in err(), k
    atlas_refusals(pt, "v3d_recon_tex_pixel_texels")
    assert pt(W=4097) == -1 and "4097" in err()
    assert pt(H=0) == -1 and "4096" in err()
    sh = calls(lib.v3d_recon_tex_shade, ("pix_tex", "pix_tw", "texture", "R", "W", "H", "b0", "b1", "b2", "image", "stream"),
               pix_tex=p, pix_tw=p, texture=p, R=64, W=32, H=32, b0=1.0, b1=1.0, b2=1.0, image=p, stream=None)
    for k in ("pix_tex", "pix_tw", "texture", "image"):
        assert sh(**{k: None}) == -1 and "v3d_recon_tex_shade:" in err() and "null" in err(), k
    assert sh(R=0) == -1 and "tex_size 0" in err()
    assert sh(R=4097) == -1 and "tex_size 4097" in err()
    assert sh(W=-3) == -1 and "4096" in err()
    assert sh(H=4097) == -1 and "4097" in err()
    tr = calls(lib.v3d_recon_tex_texel_records, ("pix_tex", "offsets", "W", "H", "n", "keys", "vals", "stream"),
               pix_tex=p, offsets=p, W=32, H=32, n=40, keys=p, vals=p, stream=None)
    for k in ("pix_tex", "offsets", "keys", "vals"):
        assert tr(**{k: None}) == -1 and "v3d_recon_tex_texel_records" in err() and "null" in err(), k
    assert tr(n=0) == -1 and "num_records 0" in err()
    assert tr(n=42) == -1 and "multiple of 4" in err()
    assert tr(n=4 * 32 * 32 + 4) == -1 and "num_records" in err()
    assert tr(W=4097) == -1 and "4096" in err()
    bw = calls(lib.v3d_recon_tex_shade_bwd, ("ranges", "ent_pix", "ent_w", "n", "dL", "W", "H", "T", "out", "stream"),
               ranges=p, ent_pix=p, ent_w=p, n=8, dL=p, W=32, H=32, T=64 * 64, out=p, stream=None)
    for k in ("ranges", "ent_pix", "ent_w", "dL", "out"):
        assert bw(**{k: None}) == -1 and "v3d_recon_tex_shade_bwd" in err() and "null" in err(), k
    assert bw(n=-1) == -1 and "negative" in err()
    assert bw(T=0) == -1 and "num_texels 0" in err()
    assert bw(T=4096 * 4096 + 1) == -1 and "num_texels" in err()
    assert bw(W=0) == -1 and "4096" in err()
    assert bw(H=5000) == -1 and "5000" in err()


# ---- the atlas ----------------------------------------------------------------------------------------------------------------------------
def _legal(F, R):
    try:
        return TX.layout(F, R)
    except ValueError:
        return None


LAYOUT_CASES = [(F, R) for F in TX.LAYOUT_F for R in TX.LAYOUT_R]


def test_layout_sizes_are_the_quoted_ones_and_small_textures_are_refused():
    from v3d_amd.recon import mesh_texture as MT
    for (F, R), S in TX.QUOTED.items():
        assert TX.layout(F, R)[0] == S == MT.atlas_layout(F, R)[0]
    legal = {c: _legal(*c) for c in LAYOUT_CASES}
    assert legal[(131_072, 1024)] == (4, 256)                                     # the largest mesh a 1024 texture takes
    assert sum(v is None for v in legal.values()) == 6 and all(legal[(F, R)] is None for F in (50_000, 131_072) for R in (64, 100, 128))
    assert legal[(131_072, 1024)] is not None and legal[(50_000, 1024)] == (6, 159)
    for (F, R), sg in legal.items():
        if sg is None:
            with pytest.raises(ValueError, match="texture too small"):
                MT.atlas_layout(F, R)
        else:
            assert MT.atlas_layout(F, R) == sg and sg[0] >= 4 and sg[1] * sg[0] <= R and 2 * sg[1] ** 2 >= F and (sg[1] == 1 or 2 * (sg[1] - 1) ** 2 < F)
    for F, R in ((0, 64), (-1, 64), (4, 0), (4, 4097)):
        with pytest.raises(ValueError):
            MT.atlas_layout(F, R)


@pytest.mark.parametrize("F,R", [c for c in LAYOUT_CASES if _legal(*c)], ids=lambda x: str(x))
def test_charts_lie_inside_the_texture_and_ownership_is_disjoint(F, R):
    S, g = TX.layout(F, R)
    L = S - 3
    vt = TX.face_uvs(F, R)
    assert float(vt.min()) >= 0 and float(vt.max()) <= g * S - 1 <= R - 1
    assert float(vt.frac().abs().max()) == 0                                       # small integers
    # both halves have the same orientation and legs of L
    e1, e2 = vt[:, 1] - vt[:, 0], vt[:, 2] - vt[:, 0]
    cross = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert bool((cross == L * L).all())
    owner, i, j = TX.texel_cells(F, R)
    count = torch.bincount(owner[owner >= 0], minlength=F)
    assert int(count.min()) >= 1 and int(count.sum()) == int((owner >= 0).sum())   # one owner per texel by construction; every face owns some
    assert set(count.unique().tolist()) <= {S * (S - 1) // 2, S * (S + 1) // 2}
    y, x = torch.div(torch.arange(R * R), R, rounding_mode="floor"), torch.arange(R * R) % R
    face = 2 * (torch.div(y, S, rounding_mode="floor") * g + torch.div(x, S, rounding_mode="floor")) + (x % S + y % S > S - 2).long()
    outside = (x >= g * S) | (y >= g * S)
    assert torch.equal(owner < 0, outside | (face >= F)) and torch.equal(owner[owner >= 0], face[owner >= 0])
    assert bool((i >= 0).all()) and bool((j >= 0).all()) and bool(((i + j)[~outside] <= S - 1).all())        # mirrored local coordinates
    # a face's corners are texels it owns
    corner = (vt[:, :, 1].long() * R + vt[:, :, 0].long())
    assert bool((owner[corner] == torch.arange(F)[:, None]).all())


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("F,R", [c for c in LAYOUT_CASES if _legal(*c)] + [(2, S) for S in range(4, 20)], ids=lambda x: str(x))
def test_no_bilinear_weight_falls_on_a_foreign_texel(F, R, dtype):
    """The footprint property: random barycentrics, the corners, the edge midpoints and the integer points of the hypotenuse of up to 64
    faces (the first, the last, random ones), through the restatement's own pixel -> texels."""
    S, g = TX.layout(F, R)
    L = S - 3
    gen = torch.Generator().manual_seed(F * 7 + R)
    faces = torch.unique(torch.cat([torch.tensor([0, F - 1, max(F - 2, 0)]), torch.randint(F, (61,), generator=gen)]))
    b = torch.rand(3000, 3, generator=gen, dtype=torch.float64) ** 2
    special = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]] + [[0, k / L, (L - k) / L] for k in range(L + 1)]
    b = torch.cat([b / b.sum(1, keepdim=True), torch.tensor(special, dtype=torch.float64)])
    n = b.shape[0]
    fid = faces.repeat_interleave(n).reshape(1, -1)
    w = (b.repeat(faces.numel(), 1) * (0.3 + torch.rand(faces.numel() * n, 1, generator=gen, dtype=torch.float64))).float().reshape(1, -1, 3)
    pt = TX.pixel_texels(fid, w, F, R, dtype)
    owner, _, _ = TX.texel_cells(F, R)
    assert bool((pt["pix_tex"] >= 0).all()) and int(pt["pix_tex"].max()) < R * R
    assert float((pt["pix_tw"].sum(-1) - 1).abs().max()) <= (1e-14 if dtype == torch.float64 else 3e-7) and float(pt["pix_tw"].min()) >= 0
    foreign = TX.foreign_weight(pt["pix_tex"], pt["pix_tw"], fid, owner)
    assert float(foreign.max()) == 0.0


# ---- the restatement's own honesty ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (TX.TEX_CASES[0], TX.TEX_CASES[9], TX.TEX_CASES[13]), ids=M.any_case_id)
def test_restatement_transpose_is_autograd_of_its_shade(case):
    v, f, c, face_id, pw = TX.case_restatement(case)
    R, F = TX.CASE_R, f.shape[0]
    pt = TX.pixel_texels(face_id, pw, F, R)
    hit = face_id >= 0
    assert bool((pt["pix_tex"][hit] >= 0).all()) and bool((pt["pix_tex"][~hit] == -1).all()) and not pt["pix_tw"][~hit].any()
    tex = TX.random_texture(R).double().requires_grad_(True)
    dL = torch.randn(3, case[3], case[2], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    assert bool((dL[:, ~hit] != 0).all())
    with torch.enable_grad():                              # (a module of the suite may have switched autograd off for the process)
        img = TX.shade(pt["pix_tex"], pt["pix_tw"], tex, RF.BG)
        (img * dL).sum().backward()
    assert torch.equal(img[:, ~hit], torch.tensor(RF.BG, dtype=torch.float64).view(3, 1).expand(3, int((~hit).sum())))
    mine = TX.shade_transpose(pt["pix_tex"], pt["pix_tw"], dL, R * R)
    assert float((mine - tex.grad).abs().max()) <= 1e-12 * float(tex.grad.abs().max())
    table, length = TX.texel_lists(pt["pix_tex"], R * R)
    assert int(length.sum()) == 4 * int(hit.sum()) and 0 < int((length == 0).sum()) < R * R
    assert not mine[length == 0].any()
    for row, n in zip(table[length > 0].tolist(), length[length > 0].tolist()):
        assert row[:n] == sorted(row[:n]) and all(x == -1 for x in row[n:])        # ascending 4 pixel + tap


def test_bake_reproduces_the_vertex_colours_at_the_corners_and_fills_the_rest():
    v, f, c = M.mesh_scene("sphere", 1)
    bad = torch.tensor([[0, 1, -1], [0, v.shape[0], 2], [2 ** 31 - 1, 1, 2]])
    ff = torch.cat([f, bad])
    for R in TX.BAKE_R:
        owner, tex = TX.bake(ff, c, R)
        vt = TX.face_uvs(ff.shape[0], R).long()
        at = tex[vt[:, :, 1] * R + vt[:, :, 0]]                                   # [F, 3, 3]
        assert float((at[:320] - c.double()[f]).abs().max()) <= 1e-15
        assert bool((tex[owner < 0] == TX.FILL).all()) and bool((tex[owner >= 320] == TX.FILL).all()) and int((owner >= 320).sum()) > 0
        assert float(tex.min()) >= 0 and float(tex.max()) <= 1


def test_restatement_loop_lowers_the_loss_on_the_end_to_end_scene():
    """GAIN of tests/test_mesh_texture_gpu.py is measured here: what the fitted texture's PSNR over all views has over the refined vertex
    colours' on the same mesh, views and schedule, in the fp64 restatement."""
    import test_mesh_texture_gpu as GPU_TESTS
    sc = TX.e2e_cpu()
    vd, fd, cd = sc["mesh"]
    assert sc["full"][1].shape[0] == 1344 and fd.shape[0] in (399, 400) and TX.layout(fd.shape[0], TX.E2E["tex_size"])[0] == 8
    res = TX.e2e_restatement(sc["mesh"], sc["targets"], sc["views"])
    tex = res["tex"]
    print(f"loss {tex['loss_first']:.4e} -> {tex['loss_last']:.4e}; PSNR vertex {res['psnr_vertex']:.2f}, baked {res['psnr_baked']:.2f}, fitted "
          f"{res['psnr_fitted']:.2f}, refined vertex colours {res['psnr_refined']:.2f} dB: gain {res['gain']:.2f} dB; {int(tex['seen'].sum())} texels seen")
    # (one view per step: a single step's loss is its view's, so the loss over ALL views is what is held, and the trend of the steps)
    print(f"mean squared error over all views {res['mse_baked']:.4e} -> {res['mse_fitted']:.4e}; first / last 8 steps "
          f"{float(np.mean(tex['losses'][:8])):.4e} / {float(np.mean(tex['losses'][-8:])):.4e}")
    # (the silhouette of 400 faces against that of 1344 is a floor no colour removes)
    assert res["mse_fitted"] < 0.75 * res["mse_baked"] and float(np.mean(tex["losses"][-8:])) < float(np.mean(tex["losses"][:8]))
    assert res["psnr_fitted"] > res["psnr_baked"] and res["psnr_fitted"] > res["psnr_refined"] > res["psnr_vertex"] - 0.5
    assert abs(res["gain"] - GPU_TESTS.RESTATEMENT_GAIN_DB) <= 0.05                 # the figure written into the GPU test
    assert 0 < int(tex["seen"].sum()) < tex["seen"].numel()
    _, baked = TX.bake(fd, cd, TX.E2E["tex_size"], torch.float32)
    assert torch.equal(tex["texture"][~tex["seen"]], baked.float().double()[~tex["seen"]])


# ---- OBJ / MTL / PNG ----------------------------------------------------------------------------------------------------------------------
def test_obj_round_trip(tmp_path):
    from v3d_amd.recon import mesh_texture as MT
    v, f, c = M.mesh_scene("sphere", 1)
    for R in (64, 100):
        vt = TX.face_uvs(f.shape[0], R, torch.float32)
        tex = TX.random_texture(R)
        path = str(tmp_path / f"m{R}.obj")
        MT.save_textured_obj(path, v, f, vt, tex)
        assert {f"m{R}.mtl", f"m{R}.obj", f"m{R}.png"} <= set(os.listdir(tmp_path))
        text = open(path).read().split("\n")
        assert text[0] == f"mtllib m{R}.mtl" and text[1] == f"usemtl m{R}" and f"map_Kd m{R}.png" in open(tmp_path / f"m{R}.mtl").read()
        # the flip, on the file itself: the first face's first corner is texel (0, 0), the TOP-left texel, so v is just below 1
        first_vt = [float(x) for x in next(line for line in text if line.startswith("vt ")).split()[1:]]
        assert first_vt == [0.5 / R, 1.0 - 0.5 / R]
        assert next(line for line in text if line.startswith("f ")) == f"f {int(f[0, 0]) + 1}/1 {int(f[0, 1]) + 1}/2 {int(f[0, 2]) + 1}/3"
        rv, rf, rvt, rtex = MT.read_textured_obj(path)
        assert rv.dtype == np.float32 and np.array_equal(rv, v.numpy()) and rf.dtype == np.int32 and np.array_equal(rf, f.numpy())
        assert rvt.dtype == np.float32 and np.array_equal(rvt, vt.numpy())
        assert rtex.shape == (R * R, 3) and float(np.abs(rtex - tex.numpy()).max()) <= 0.5 / 255 + 1e-7
        from PIL import Image
        img = np.asarray(Image.open(tmp_path / f"m{R}.png"))
        assert img.shape == (R, R, 3) and abs(int(img[3, 5, 1]) - 255 * float(tex[3 * R + 5, 1])) <= 0.5 + 1e-4        # row y, column x
    with pytest.raises(ValueError, match="not a square"):
        MT.save_textured_obj(str(tmp_path / "bad.obj"), v, f, vt, torch.zeros(10, 3))
    with pytest.raises(ValueError, match="texture coordinates"):
        MT.save_textured_obj(str(tmp_path / "bad.obj"), v, f, vt[:5], tex)


# ---- the script and the host API ----------------------------------------------------------------------------------------------------------
def _entry(name):
    spec = importlib.util.spec_from_file_location("v3d_entry_" + name, os.path.join(ROOT, "scripts", "pub", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_options_parse_with_the_reconstructions_defaults():
    mod = _entry("texture_mesh")
    ap = mod.build_parser()
    a = vars(ap.parse_args(["--mesh", "out/gs/mesh.ply", "--video", "out/000000.npy", "-o", "out/gs/mesh.obj", "-w"]))
    assert a == {"mesh": "out/gs/mesh.ply", "video": "out/000000.npy", "out": "out/gs/mesh.obj", "white_background": True, "texture_resolution": 1024,
                 "iters": 2000, "num_opt": 0, "lr": 1e-3, "seed": 0, "num_frames": None, "radius": 2.0, "elevation": 0.0, "fov": 60.0, "render_orbit": 0}
    recon = vars(_entry("recon_from_vid").build_parser().parse_args(["--video", "x.npy"]))
    for k in ("radius", "elevation", "fov", "seed", "num_frames", "white_background"):
        assert vars(ap.parse_args(["--mesh", "m.ply", "--video", "x.npy"]))[k] == recon[k], k
    for bad in (["--video", "x.npy"], ["--mesh", "m.ply"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    base = ["--mesh", "does/not/exist.ply", "--video", "does/not/exist.npy"]
    for bad in (["--texture_resolution", "0"], ["--texture_resolution", "4097"], ["--iters", "-1"], ["--num_opt", "-2"], ["--lr", "-0.1"],
                ["-o", "out.ply"], ["--render_orbit", "-1"]):
        with pytest.raises(SystemExit):                    # refused before anything is read
            mod.main(base + bad)


def test_host_api_refuses_what_does_not_fit_and_answers_the_empty_mesh_without_a_launch():
    from v3d_amd.recon import mesh_texture as MT
    cams = D.cams_for(32, 32)
    v, f = M.icosphere(0)
    c = M.position_colors(v)
    with pytest.raises(ValueError, match="does not match"):
        MT.fit_texture(v, f, c, cams, torch.zeros(4, 3, 32, 40), device="cpu")
    with pytest.raises(ValueError, match="3 images for 4 cameras"):
        MT.fit_texture(v, f, c, cams, torch.zeros(3, 3, 32, 32), device="cpu")
    with pytest.raises(ValueError, match="outside the vertex array"):
        MT.prepare_texture_view(cams[0], v, f + 1, 64, [1, 1, 1], device="cpu")
    with pytest.raises(ValueError, match="texture too small for 20 faces"):
        MT.prepare_texture_view(cams[0], v, f, 15, [1, 1, 1], device="cpu")
    with pytest.raises(ValueError, match="texture too small"):
        MT.bake_vertex_colors(f, c, 15, device="cpu")
    with pytest.raises(ValueError, match="texture too small"):
        MT.face_uvs(20, 15, device="cpu")
    with pytest.raises(ValueError, match="tex_size 5000"):
        MT.fit_texture(v, f, c, cams, torch.zeros(4, 3, 32, 32), tex_size=5000, device="cpu")
    # V = 0 / F = 0: the background, the fill, zero gradients, no launch (so it runs here)
    R = 16
    assert tuple(MT.face_uvs(0, R, device="cpu").shape) == (0, 3, 2)
    for vv, ff in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64)), (v, torch.zeros(0, 3, dtype=torch.int64))):
        view = MT.prepare_texture_view(D.cams_for(56, 40)[0], vv, ff, R, [0.25, 0.5, 1.0], device="cpu")
        assert not view.launch and view.ent_pix.numel() == 0 and tuple(view.ranges.shape) == (R * R, 2) and bool((view.pix_tex == -1).all())
        tex = torch.rand(R * R, 3, requires_grad=True)
        with torch.enable_grad():                          # (a module of the suite may have switched autograd off for the process)
            img = MT.texture_shade(view, tex)
            (img * torch.rand(3, 40, 56)).sum().backward()
        assert img.shape == (3, 40, 56) and torch.equal(img[:, 7, 9], torch.tensor([0.25, 0.5, 1.0]))
        assert tex.grad.shape == tex.shape and not tex.grad.any()
        owner, baked = MT.bake_vertex_colors(ff, torch.rand(vv.shape[0], 3), R, device="cpu")
        assert bool((owner == -1).all()) and bool((baked == MT.FILL).all())
        out, stats = MT.fit_texture(vv, ff, torch.rand(vv.shape[0], 3), D.cams_for(56, 40), torch.ones(4, 3, 40, 56), tex_size=R, iterations=5, device="cpu")
        assert torch.equal(out, baked) and stats["texels_seen"] == 0 and stats["loss_first"] is None
        assert stats["psnr_vertex"] == stats["psnr_baked"] == stats["psnr_fitted"] == float("inf") and stats["opt_views"] == [0, 1, 2, 3]


# ---- the premises of the GPU cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TX.TEX_CASES, ids=M.any_case_id)
def test_premises_of_the_gpu_cases(case):
    """On the restatement alone: with R = CASE_R every case leaves at most 2 % of its covered pixels out of the exact comparison of
    pix_tex, the float32 restatement agrees with the fp64 one on the pixels kept, and the fp64 foreign weight is exactly 0."""
    v, f, c, face_id, pw = TX.case_restatement(case)
    R, F = TX.CASE_R, f.shape[0]
    p64, p32 = TX.pixel_texels(face_id, pw, F, R), TX.pixel_texels(face_id, pw, F, R, torch.float32)
    keep, out = TX.compared_taps(p64, TX.TAP_MARGIN)
    print(f"{M.any_case_id(case)}: {int((face_id >= 0).sum())} covered pixels, {100 * out:.3f} % left out")
    assert int((face_id >= 0).sum()) > 0 and out <= M.EXCLUDE_MAX
    assert torch.equal(p32["pix_tex"][keep], p64["pix_tex"][keep])
    owner, _, _ = TX.texel_cells(F, R)
    assert float(TX.foreign_weight(p64["pix_tex"], p64["pix_tw"], face_id, owner).max()) == 0.0


def test_premises_of_the_long_list_and_synthetic_cases():
    ranges, ent_pix, ent_w, dL = TX.synthetic_lists()
    assert (ranges[:, 1] - ranges[:, 0]).tolist() == [0, 1, 2, 63, 64, 65, 700, 0] and int(ent_pix.max()) < 64 * 48
    assert bool((ent_w > 0).any()) and bool((ent_w < 0).any())                     # mixed sign
    # the full-image quad at R = 8: F = 2 -> one cell of S = 8, 64 x 48 pixels over at most 36 texels a face
    q, zv, faces, _ = RF.full_quad(64, 48)
    assert TX.layout(2, 8) == (8, 1)
    fid = torch.zeros(48, 64, dtype=torch.long)
    fid[torch.arange(48)[:, None] * 64 > torch.arange(64)[None, :] * 48] = 1          # below the diagonal: face 1 (0, 3, 2)
    _, pw = RF.pixel_weights(q, zv, faces, fid, 8, torch.float32)
    _, length = TX.texel_lists(TX.pixel_texels(fid, pw, 2, 8)["pix_tex"], 64)
    assert int(length.max()) > 300 and int(length.sum()) == 4 * 64 * 48

"""The shading kernels of csrc/meshshade.hip, the Renderer's autograd nodes over them and the shaded training renders of
TexturedMeshModel, against the float64 reference of tests/meshshade_reference.py.

The reference takes the GPU's own face_idx (and, for the pixel kernels, the GPU's own barycentrics: they are inputs);
tests/test_meshshade_cpu.py asserts that no other decision of these scenes sits on a rounding edge.  Tolerances: for every
compared tensor the same reference was run in float32 on the CPU on these very inputs, and 4 x its largest deviation from
float64 (relative to the tensor's largest magnitude) is allowed -- REL below, printed by

    python -m tests.meshshade_reference

A row "shade_<n><l><d>_<H>x<W>" is the pixel kernels' with only the marked incoming gradients (normal, lighting, depth)
present; its six figures are normal, lighting, depth, grad_bary, grad_vnormals, grad_face_z.  The results with one writer
per element are also compared bit for bit (run against run, and a NULL gradient against a gradient of zeros); the two sums
the backward adds into with float atomics depend on the order of the additions, so they are held to the tolerance and,
where a gradient is absent, to exact zeros."""
import math
import os
import types

import pytest
import torch

from tests import meshshade_reference as MS
from tests import rastergrad_reference as RG

pytestmark = pytest.mark.gpu

REL = {
    'vnormals_tetra': (7.82e-08, 2.9e-07),
    'vnormals_fan': (7.02e-08, 1.16e-07),
    'vnormals_ico1': (8.6e-08, 1.01e-07),
    'vnormals_ico3': (1.22e-07, 1.26e-07),
    'vnormals_fan_edges': (7.02e-08, 1.39e-07),
    'shade_111_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 1.03e-07, 1.7e-07, 2.03e-07),
    'shade_110_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 1.25e-07, 1.7e-07, 0),
    'shade_101_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 1.1e-07, 1.54e-07, 2.03e-07),
    'shade_100_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 1.73e-07, 1.54e-07, 0),
    'shade_011_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 5.87e-08, 1.84e-07, 2.03e-07),
    'shade_010_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 1.52e-07, 1.84e-07, 0),
    'shade_001_16x16': (1.15e-07, 1.35e-07, 6.89e-08, 3.62e-08, 0, 2.03e-07),
    'shade_111_13x11': (1e-07, 8.09e-08, 7.11e-08, 5.18e-08, 1.85e-07, 8.26e-08),
    'shade_110_13x11': (1e-07, 8.09e-08, 7.11e-08, 1.03e-07, 1.85e-07, 0),
    'shade_101_13x11': (1e-07, 8.09e-08, 7.11e-08, 8.15e-08, 3e-07, 8.26e-08),
    'shade_100_13x11': (1e-07, 8.09e-08, 7.11e-08, 1.17e-07, 3e-07, 0),
    'shade_011_13x11': (1e-07, 8.09e-08, 7.11e-08, 3.49e-08, 1.12e-07, 8.26e-08),
    'shade_010_13x11': (1e-07, 8.09e-08, 7.11e-08, 1.44e-07, 1.12e-07, 0),
    'shade_001_13x11': (1e-07, 8.09e-08, 7.11e-08, 2.85e-08, 0, 8.26e-08),
    'sphere_chain': (5.96e-06, 3.5e-07, 1.4e-07, 2.04e-07, 2.4e-06),
    'sphere_reason': (9.48e-08, 3.5e-07, 1.4e-07, 2.04e-07, 1.15e-06),
}
POISON = 7.0


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _d(t, dev, dtype=torch.float32):
    """A contiguous device copy the caller keeps alive across the launch."""
    return t.to(dtype).contiguous().to(dev)


def _lib():
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    return _b, _p


def _close(name, got, want, rel):
    """|got - want| <= tolerance(rel, max|want|); prints the figure first."""
    mag = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    tol = RG.tolerance(rel, mag)
    print("%s: max error %.3g, allowed %.3g (magnitude %.3g)" % (name, err, tol, mag))
    assert mag > 0 and err <= tol, (name, err, tol)


def _finite(*tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


# ------------------------------------------------------------------------------------------------ vertex normals
def _table(dev, faces, V):
    from src.latent_paint.models.render import corner_table
    return corner_table(faces.to(dev), V)


def _vn_forward(dev, verts, faces, table=None):
    _b, _p = _lib()
    V, F = verts.shape[0], faces.shape[0]
    verts_d, faces_d = _d(verts, dev), _d(faces, dev, torch.int32)
    start, corners = _table(dev, faces, V) if table is None else table
    vn = torch.full((V, 3), POISON, device=dev)
    _b.call("lnerf_vertex_normals_forward", _p(verts_d), V, _p(faces_d), F, _p(start), _p(corners), _p(vn), None)
    return vn


def _vn_backward(dev, verts, faces, gvn):
    _b, _p = _lib()
    V, F = verts.shape[0], faces.shape[0]
    verts_d, faces_d, gvn_d = _d(verts, dev), _d(faces, dev, torch.int32), _d(gvn, dev)
    start, corners = _table(dev, faces, V)
    need = _b.get_lib().lnerf_vertex_normals_scratch_bytes(V, F)
    scratch = torch.full((need,), 0x7f, device=dev, dtype=torch.uint8)
    gv = torch.full((V, 3), POISON, device=dev)                           # OVERWRITTEN
    _b.call("lnerf_vertex_normals_backward", _p(gvn_d), _p(verts_d), V, _p(faces_d), F, _p(start), _p(corners),
            _p(scratch), need, _p(gv), None)
    return gv


@pytest.mark.parametrize("name", ("tetra", "fan", "ico1", "ico3"))
def test_vertex_normals_and_their_gradient_match_the_reference_with_the_same_bits_on_every_run(dev, name):
    verts, faces = MS.normal_meshes()[name]
    gvn = MS.randn(tuple(verts.shape), 42)
    want_vn, want_gv = MS.case_vnormals(faces)(verts.clone(), gvn)
    vn, gv = _vn_forward(dev, verts, faces), _vn_backward(dev, verts, faces, gvn)
    rel = REL["vnormals_" + name]
    _close("vertex normals " + name, vn, want_vn, rel[0])
    _close("vertex normals grad_verts " + name, gv, want_gv, rel[1])
    assert torch.equal(_vn_forward(dev, verts, faces), vn) and torch.equal(_vn_backward(dev, verts, faces, gvn), gv)
    assert float((vn.norm(dim=1) - 1).abs().max()) < 1e-6


def test_vertex_normal_edge_cases_give_the_stated_zeros_and_move_nothing_else(dev):
    verts, faces, zero = MS.fan_edge_mesh()
    gvn = MS.randn(tuple(verts.shape), 42)
    want_vn, want_gv = MS.case_vnormals(faces)(verts.clone(), gvn)
    vn, gv = _vn_forward(dev, verts, faces), _vn_backward(dev, verts, faces, gvn)
    assert _finite(vn, gv)
    assert bool((vn[zero] == 0).all()) and bool((gv[zero] == 0).all())
    _close("edge cases: vertex normals", vn, want_vn, REL["vnormals_fan_edges"][0])
    _close("edge cases: grad_verts", gv, want_gv, REL["vnormals_fan_edges"][1])
    fan_v, fan_f = MS.fan_mesh()
    assert torch.equal(vn[:8], _vn_forward(dev, fan_v, fan_f))            # the fan's own normals: the same bits
    assert torch.equal(gv[:8], _vn_backward(dev, fan_v, fan_f, gvn[:8]))
    assert torch.equal(_vn_forward(dev, verts, faces), vn) and torch.equal(_vn_backward(dev, verts, faces, gvn), gv)


def test_a_wrong_corner_table_gives_wrong_normals_and_reads_nothing_out_of_range(dev):
    """Entries that are no corner of their vertex (another vertex's corners, -1, 3F) are skipped, and corner_start is
    clamped into the list: every vertex of a table shifted by one vertex sums nothing."""
    verts, faces = MS.fan_mesh()
    V, F3 = verts.shape[0], faces.numel()
    start, corners = _table(dev, faces, V)
    shifted = torch.cat([start[1:], start[-1:]]).contiguous()             # vertex i is handed vertex i + 1's corners
    assert float(_vn_forward(dev, verts, faces, (shifted, corners)).abs().max()) == 0.0
    junk = torch.tensor([-1, F3, F3 + 7, -5] * (F3 // 4 + 1), dtype=torch.int32, device=dev)[:F3].contiguous()
    assert float(_vn_forward(dev, verts, faces, (start, junk)).abs().max()) == 0.0
    wild = torch.tensor([-9] + [F3 + 100] * V, dtype=torch.int32, device=dev)   # every range clamps into [0, 3F]
    got = _vn_forward(dev, verts, faces, (wild, corners))
    assert _finite(got) and torch.equal(got[1:], torch.zeros_like(got[1:]))


# ------------------------------------------------------------------------------------------------ pixel shading
@pytest.fixture(scope="module", params=RG.SIZES, ids=lambda s: "%dx%d" % s)
def pix(request, dev):
    """RG.screen_scene() at one size, rasterised once on the GPU, with MS.pixel_scene's normals, lights and gradients."""
    _b, _p = _lib()
    H, W = request.param
    fxy, fz, faces = RG.screen_scene()
    B, F = fz.shape[0], fz.shape[1]
    fxy_d, fz_d = _d(fxy, dev), _d(fz, dev)
    box = torch.tensor([0, W - 1, 0, H - 1], dtype=torch.int16).repeat(B, F, 1).contiguous().to(dev)
    idx_d = torch.full((B * H * W,), -9, dtype=torch.int32, device=dev)
    bary_d = torch.full((B * H * W, 3), POISON, device=dev)
    _b.call("lnerf_rasterize_batch", B, H, W, _p(fz_d), _p(fxy_d), _p(box), F, _p(idx_d), _p(bary_d), None)
    idx = idx_d.cpu().long()
    assert torch.equal(idx, RG.oracle_face_idx(fxy, fz, H, W))            # the winners the CPU preconditions were checked on
    s = MS.pixel_scene(H, W, face_idx=idx)
    s["bary"] = bary_d.cpu().double()                                     # the kernel's own input
    s.update(key="%dx%d" % (H, W), B=B, F=F, V=19, idx_d=idx_d, bary_d=bary_d, fz_d=fz_d,
             faces_d=_d(faces, dev, torch.int32), vn_d=_d(s["vn"], dev), lights_d=_d(s["lights"], dev),
             grads_d=[_d(s[k], dev) for k in ("gn", "gl", "gd")])
    return s


def _shade_forward(s, dev, outputs=(1, 1, 1)):
    _b, _p = _lib()
    P = s["B"] * s["H"] * s["W"]
    outs = [torch.full(shape, POISON, device=dev) if on else None
            for shape, on in zip(((P, 3), (P,), (P,)), outputs)]
    _b.call("lnerf_raster_shade_forward", _p(s["idx_d"]), _p(s["bary_d"]), _p(s["fz_d"]), _p(s["faces_d"]), _p(s["vn_d"]),
            _p(s["lights_d"]), s["B"], s["H"], s["W"], s["F"], s["V"], *[_p(o) for o in outs], None)
    return outs


def _shade_backward(s, dev, grads, fill=0.0):
    """grads: the three incoming gradients (None: a NULL pointer) -> (grad_bary, grad_vnormals, grad_face_z)."""
    _b, _p = _lib()
    P = s["B"] * s["H"] * s["W"]
    gbary = torch.full((P, 3), POISON, device=dev)                        # OVERWRITTEN
    gvn = torch.full((s["V"], 3), fill, device=dev)                       # ADDED INTO
    gz = torch.full((s["B"], s["F"], 3), fill, device=dev)                # ADDED INTO
    _b.call("lnerf_raster_shade_backward", *[_p(g) for g in grads], _p(s["idx_d"]), _p(s["bary_d"]), _p(s["fz_d"]),
            _p(s["faces_d"]), _p(s["vn_d"]), _p(s["lights_d"]), s["B"], s["H"], s["W"], s["F"], s["V"], _p(gbary),
            _p(gvn), _p(gz), None)
    return gbary, gvn, gz


def _reference(s, combo=(1, 1, 1)):
    return MS.case_shade(s["idx"], s["faces"], s["H"], s["W"], combo)(
        s["vn"].clone(), s["bary"].clone(), s["fz"].clone(), s["lights"], s["gn"], s["gl"], s["gd"])


def test_shading_forward_matches_the_reference_and_writes_every_element(pix, dev):
    s = pix
    want = _reference(s)[:3]
    outs = _shade_forward(s, dev)
    rel = REL["shade_111_" + s["key"]]
    for name, got, w, r in zip(("normal", "lighting", "depth"), outs, want, rel):
        assert bool((got != POISON).all())                                # every element was written
        _close("shade %s %s" % (name, s["key"]), got, w, r)
        assert bool((got[s["idx_d"] < 0] == 0).all())                     # background holds 0
    normal, lighting, depth = outs
    fg = s["idx_d"] >= 0
    assert float((normal[fg].norm(dim=1) - 1).abs().max()) < 1e-6 and bool((depth[fg] > 0).all())
    view0, view1 = lighting[:s["H"] * s["W"]], lighting[s["H"] * s["W"]:]
    assert int((view0 == 1e-8).sum()) >= 8 and int((view1 == 1.0).sum()) >= 8 and float(view0.max()) < 1.0
    assert bool((lighting[fg] >= 1e-8).all()) and bool((lighting <= 1.0).all())
    # the same bits on every run, and with any output left out
    for combo in MS.COMBOS:
        for a, b in zip(_shade_forward(s, dev, combo), outs):
            assert a is None or torch.equal(a, b), combo


@pytest.mark.parametrize("combo", MS.COMBOS, ids=lambda c: "%d%d%d" % c)
def test_shading_backward_matches_the_reference_under_every_combination_of_gradients(pix, dev, combo):
    s = pix
    want = _reference(s, combo)[3:]
    grads = [g if on else None for g, on in zip(s["grads_d"], combo)]
    got = _shade_backward(s, dev, grads)
    rel = REL["shade_%d%d%d_%s" % (*combo, s["key"])][3:]
    assert _finite(*got) and bool((got[0] != POISON).all())
    for name, g, w, r in zip(("grad_bary", "grad_vnormals", "grad_face_z"), got, want, rel):
        if float(w.abs().max()) == 0:                                     # no gradient reaches it: exactly nothing is added
            assert float(g.abs().max()) == 0.0, name
        else:
            _close("shade %s %s %s" % (name, combo, s["key"]), g, w, r)
    gbary, gvn, gz = got
    assert bool((gbary[s["idx_d"] < 0] == 0).all())
    assert float(gvn[13:].abs().max()) == 0.0 and float(gz[:, 8:].abs().max()) == 0.0   # faces that never win: nothing
    # a NULL gradient is a gradient of zeros: grad_bary (one writer) bit for bit, on every run
    zeros = [g if on else torch.zeros_like(g) for g, on in zip(s["grads_d"], combo)]
    assert torch.equal(_shade_backward(s, dev, zeros)[0], gbary)
    # grad_vnormals and grad_face_z are ADDED INTO: what no pixel reaches keeps its value
    _, gvn1, gz1 = _shade_backward(s, dev, grads, fill=1.0)
    assert bool((gvn1[13:] == 1).all()) and bool((gz1[:, 8:] == 1).all())
    # ... and the rest is 1 + the sum, not the sum: overwriting would be off by 1.  (The sum itself was compared above; from 1
    # every one of up to P additions rounds at the size of its partial sum, below 2^-24 (1 + sum |terms|) each, and
    # sum |terms| <= P max|term| is not known here, so this is a check of the property at 1e-3, not of the precision.)
    for name, added, alone in (("grad_vnormals", gvn1, gvn), ("grad_face_z", gz1, gz)):
        assert float(((added - 1) - alone).abs().max()) <= 1e-3 * (1 + float(alone.abs().max())), name


def test_clamped_pixels_pass_no_gradient_through_the_lighting(pix, dev):
    s = pix
    info = {}
    MS.shade(s["idx"], s["bary"], s["fz"], s["faces"], s["vn"], s["lights"], s["H"], s["W"], info)
    clamped = info["fg"] & ((info["unclamped"] < MS.LIGHT_MIN) | (info["unclamped"] > MS.LIGHT_MAX))
    assert int(clamped.sum()) >= 16
    gl = torch.where(clamped, s["gl"], torch.zeros_like(s["gl"]))
    gbary, gvn, gz = _shade_backward(s, dev, [None, _d(gl, dev), None])
    assert float(gvn.abs().max()) == 0.0 and float(gbary.abs().max()) == 0.0 and float(gz.abs().max()) == 0.0
    gl = torch.where(clamped, torch.zeros_like(s["gl"]), s["gl"])          # and the others do
    assert float(_shade_backward(s, dev, [None, _d(gl, dev), None])[1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the whole chain
def _render_sphere(dev, constant, antialias):
    """The sphere scene through the Renderer -> (verts leaf, image [B,H,W,C+1] with the lighting in, its unshaded twin,
    normal [B,H,W,3], lighting, depth [B,H,W], face_idx, the scene)."""
    from src.latent_paint.models.render import Renderer
    scene = MS.sphere_scene(constant)
    verts, faces, cams, face_uv, tex, lights = scene
    S = MS.SPHERE_SIDE
    r = Renderer(dev, dim=(S, S), interpolation_mode="bilinear", antialias=antialias)
    vd = verts.float().to(dev).requires_grad_()
    elev, azim, rad = zip(*MS.SPHERE_VIEWS)
    img, mask, state = r.render_views_texture(vd, faces.to(dev), face_uv.float().to(dev)[None], tex.float().to(dev)[None],
                                              elev, azim, rad, look_at_height=0.0, return_state=True)
    normal, lighting, depth = r.shade_views(vd, faces.to(dev), state)
    assert normal.shape == (2, 3, S, S) and lighting.shape == (2, 1, S, S) and depth.shape == (2, 1, S, S)
    shaded, plain = torch.cat([img * lighting, mask], 1), torch.cat([img, mask], 1)
    if antialias:
        shaded = r.antialias_views(shaded, state, faces.to(dev))
    idx = state.face_idx.cpu().long()
    assert torch.equal(idx, MS.sphere_winners(verts, faces, cams))
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    return vd, nhwc(shaded), nhwc(plain), nhwc(normal), lighting[:, 0], depth[:, 0], idx, scene


@pytest.fixture(scope="module")
def chain(dev):
    vd, shaded, _, normal, lighting, depth, idx, scene = _render_sphere(dev, constant=False, antialias=True)
    w = MS.sphere_weights(shaded.shape[-1])
    w1, w2, w3 = (t.float().to(dev) for t in w)
    (gv,) = torch.autograd.grad((shaded * w1).sum() + (normal * w2).sum() + (depth * w3).sum(), vd)
    want = MS.case_sphere(idx, scene[1], True)(scene[0].clone(), *scene[2:], *w)
    return (shaded.detach(), normal.detach(), lighting.detach(), depth.detach(), gv), want, idx, scene


def test_whole_chain_vertices_to_shaded_image_normals_and_depth(chain):
    got, want, _, _ = chain
    for name, g, w, r in zip(("image", "normal", "lighting", "depth", "grad_verts"), got, want, REL["sphere_chain"]):
        _close("sphere chain " + name, g, w, r)
    inner = MS.interior_vertices(chain[2], chain[3][1], 42)
    assert len(inner) >= 3 and bool((want[4][inner].abs().amax(1) > 0).all())


def test_the_chain_comparison_bites_on_one_vertex(chain):
    got, want, idx, scene = chain
    broken = got[4].clone()
    broken[MS.interior_vertices(idx, scene[1], 42)[0]] = 0
    with pytest.raises(AssertionError):
        _close("sphere chain grad_verts, one vertex zeroed", broken, want[4], REL["sphere_chain"][4])


def test_without_a_graph_shade_views_launches_the_two_forward_kernels_only(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_paint.models.render import Renderer
    verts, faces, cams, face_uv, tex, lights = MS.sphere_scene()
    S = MS.SPHERE_SIDE
    r = Renderer(dev, dim=(S, S), interpolation_mode="bilinear")
    elev, azim, rad = zip(*MS.SPHERE_VIEWS)
    vd = verts.float().to(dev)
    state = r._rasterize_views_faces(vd, faces.to(dev), elev, azim, rad, 0.0, (S, S))
    calls = []
    _b.set_profile_hook(lambda name, when: calls.append(name) if when == "pre" else None)
    try:
        plain = r.shade_views(vd, faces.to(dev), state)
        with torch.no_grad():
            quiet = r.shade_views(vd.clone().requires_grad_(), faces.to(dev), state, lights=MS.DEFAULT_LIGHTS)
    finally:
        _b.set_profile_hook(None)
    assert calls == ["lnerf_vertex_normals_forward", "lnerf_raster_shade_forward"] * 2
    assert all(t.grad_fn is None and not t.requires_grad for t in plain + quiet)
    assert all(torch.equal(a, b) for a, b in zip(plain, quiet))
    rows = torch.tensor([[2 * v for v in MS.DEFAULT_LIGHTS], MS.DEFAULT_LIGHTS], device=dev)   # view 0 faces the light
    per_view = r.shade_views(vd, faces.to(dev), state, lights=rows)[1]
    assert torch.equal(per_view[1], plain[1][1]) and float(per_view[0].max()) == 1.0 and float(plain[1].max()) < 1.0
    for bad in ((1.0, 0.0), [float("nan")] * 9, torch.zeros(3, 9)):
        with pytest.raises(ValueError):
            r.shade_views(vd, faces.to(dev), state, lights=bad)
    assert len(r._corners) == 1                                           # the corner table is made once per mesh


def test_the_reason_for_the_feature(dev):
    """Constant texture, no antialiasing: the image alone gives the vertices exactly no gradient; image * lighting gives
    the interior vertices one, and it is the reference's."""
    vd, shaded, plain, _, lighting, _, idx, scene = _render_sphere(dev, constant=True, antialias=False)
    w = MS.sphere_weights(shaded.shape[-1])
    w1 = w[0].float().to(dev)
    (g_plain,) = torch.autograd.grad((plain * w1).sum(), vd, retain_graph=True)
    assert float(g_plain.abs().max()) == 0.0
    (g_shaded,) = torch.autograd.grad((shaded * w1).sum(), vd)
    want = MS.case_sphere(idx, scene[1], False, (1, 0, 0))(scene[0].clone(), *scene[2:], *w)
    _close("reason: image", shaded.detach(), want[0], REL["sphere_reason"][0])
    _close("reason: grad_verts", g_shaded, want[4], REL["sphere_reason"][4])
    lit = lighting.detach().reshape(-1).cpu()
    inner = MS.interior_vertices(idx, scene[1], 42, keep=(lit > 1e-8) & (lit < 1.0))   # (a clamped lighting passes nothing)
    assert len(inner) >= 3 and bool((g_shaded[inner].abs().amax(1) > 0).all())


# ------------------------------------------------------------------------------------------------ model and trainer
VIEWS = ([math.radians(70.0), math.radians(100.0)], [0.3, 2.4], [1.3, 1.25])
GEOMETRY = {"optim.disp_lr": 5e-5, "render.antialias": True, "guide.texture_interpolation_mode": "bilinear"}


def _cfg(tmp_path, obj, **over):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "shade", "log.exp_root": str(tmp_path), "guide.text": "a goldfish", "guide.shape_path": obj,
            "guide.texture_resolution": 16, "render.train_grid_size": 16}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat).validate()


def _model(cfg, dev, seed=0):
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    torch.manual_seed(seed)
    return TexturedMeshModel(cfg, device=dev, render_grid_size=cfg.render.train_grid_size, latent_mode=True,
                             texture_resolution=cfg.guide.texture_resolution).to(dev)


@pytest.fixture(scope="module")
def sphere_obj(tmp_path_factory):
    return MS.write_sphere_obj(tmp_path_factory.mktemp("shade_mesh") / "sphere.obj", subdiv=2)


def test_albedo_is_what_a_model_without_the_new_fields_renders(dev, tmp_path, sphere_obj):
    cfg = _cfg(tmp_path, sphere_obj)
    old = types.SimpleNamespace(log=cfg.log, guide=cfg.guide, optim=cfg.optim, render=types.SimpleNamespace(
        **{k: v for k, v in vars(cfg.render).items() if k not in ("shading", "shading_ratio", "lights")}))
    assert not hasattr(old.render, "shading")
    a, b = _model(cfg, dev).render(*VIEWS), _model(old, dev).render(*VIEWS)
    assert set(a) == set(b) == {"image", "mask", "background", "foreground"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    off = _model(_cfg(tmp_path, sphere_obj, **{"render.shading": "lambertian", "render.shading_ratio": 0.0}), dev)
    for _ in range(2):
        c = off.render(*VIEWS)
        assert set(c) == set(a) and all(torch.equal(a[k], c[k]) for k in a)
    test = _model(cfg, dev).render(*VIEWS, decode_func=lambda t: t[:, :3], test=True, dims=(24, 24), maps=True)
    assert test["normal"].shape == (2, 3, 24, 24) and test["lighting"].shape == test["depth"].shape == (2, 1, 24, 24)
    assert set(_model(cfg, dev).render(*VIEWS, decode_func=lambda t: t[:, :3], test=True, dims=(24, 24))) == \
        {"image", "texture_map", "mask"}


def test_lambertian_renders_carry_the_maps_and_move_the_interior_vertices(dev, tmp_path, sphere_obj):
    m = _model(_cfg(tmp_path, sphere_obj, **{**GEOMETRY, "render.shading": "lambertian"}), dev)
    with torch.no_grad():
        m.texture_img.fill_(0.625)                                        # constant: no gradient through the UVs
    out = m.render(*VIEWS)
    assert set(out) == {"image", "mask", "background", "foreground", "normal", "lighting", "depth", "shading",
                        "geometry_loss"}
    assert out["shading"] == "lambertian" and out["image"].shape == (2, 4, 64, 64)
    assert out["normal"].shape == (2, 3, 16, 16) and out["lighting"].shape == out["depth"].shape == (2, 1, 16, 16)
    g = torch.randn(out["image"].shape, generator=torch.Generator().manual_seed(3)).to(dev)
    out["image"].backward(gradient=g)
    grad = m.displacement.grad
    assert _finite(grad) and float(grad.abs().max()) > 0
    view = m._view(*VIEWS)
    state = m.renderer._rasterize_views_faces(m.mesh.vertices, m.mesh.faces, view["elev"], view["azim"], view["radius"],
                                              view["look_at_height"], (16, 16))
    lit = out["lighting"].detach().reshape(-1).cpu()                       # (a clamped lighting passes no gradient)
    inner = MS.interior_vertices(state.face_idx.cpu().long(), m.mesh.faces.cpu(), grad.shape[0],
                                 keep=(lit > 1e-8) & (lit < 1.0))
    print("interior vertices under an unclamped lighting: %d of %d" % (len(inner), grad.shape[0]))
    assert len(inner) >= 3 and bool((grad[inner].abs().amax(1) > 0).all())
    # the RGB backbone: textureless is the lighting on three channels
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    cfg = _cfg(tmp_path, sphere_obj, **{"render.shading": "textureless", "render.backbone": "texture-rgb-mesh"})
    rgb = TexturedMeshModel(cfg, device=dev, render_grid_size=16, latent_mode=False, texture_resolution=16).to(dev)
    grey = rgb.render(*VIEWS)
    assert grey["shading"] == "textureless" and grey["image"].shape == (2, 3, 16, 16)
    assert torch.equal(grey["foreground"], grey["lighting"].expand(-1, 3, -1, -1))


def test_three_trainer_steps_under_lambertian_shading_write_the_evaluation_maps(dev, tmp_path, sphere_obj):
    from src.latent_paint.training.trainer import Trainer
    over = {"render.shading": "lambertian", "render.batch_size": 2, "optim.iters": 3, "log.save_interval": 3,
            "log.eval_size": 1, "log.full_eval_size": 1, "log.eval_maps": True, "log.save_mesh": False,
            "render.eval_grid_size": 32}
    tr = Trainer(_cfg(tmp_path, sphere_obj, **over), device=dev)
    before = tr.mesh_model.texture_img.detach().clone()
    tr.train()
    assert tr.train_step == 3 and not torch.equal(tr.mesh_model.texture_img.detach(), before)
    assert _finite(tr.mesh_model.texture_img.detach())
    vis = tmp_path / "shade" / "vis" / "eval"
    for step in (0, 3):
        for kind in ("rgb", "normals", "depth", "shaded"):
            assert os.path.exists(vis / ("step_%05d_0000_%s.png" % (step, kind))), (step, kind)
    from PIL import Image
    import numpy as np
    depth = np.asarray(Image.open(vis / "step_00003_0000_depth.png"))
    assert depth.shape == (32, 32, 3) and depth.max() == 255 and depth.min() == 0   # near is bright, background is 0

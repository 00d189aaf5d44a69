"""Known-answer hits at every branch of the shading arithmetic, in 3-D .. 12-D.

ndt_amd/csrc/ndt_shading.hpp (surface_of, shadow_lit, light_term, children_of, blend_children, shadow_dir), light_setup in
ndt_kernels.hip and v_refract / v_reflect / v_angle in ndt_device.hpp are compiled once per dimension.  The fixtures shade3d ..
shade12d (tests/scenes/parity_shade.c, rendered by the compiled reference: tests/golden/make_golden_shade.py) are one 48x27
frame at depth 8 per dimension, with and without specular lighting, built so that every branch of apply_lights (ndt.c:71-326),
get_ray_color (ndt.c:329-450) and vectNd_refract (vectNd.c:119-188) is taken in every dimension.  That they are is not left to
the scene's comments: this file restates the shading in numpy long double, walking every pixel's tree level by level, counts
every branch and asserts the counts (COVERAGE below).

The restatement takes its primary rays from test_view_modes.model_rays in long double and its intersections (closest hits and
shadow answers) from oracle.trace, which other files hold to the reference; everything between -- light setup, the same-side
test, the cone test, lit or shadowed, the diffuse and specular terms, the children and their cut-offs, vectNd_reflect,
vectNd_refract, the blend -- is evaluated in a 64-bit mantissa.  Every decision records its margin; a pixel with a decision
closer than FRAGILE to its threshold is left out of the frame comparisons (an exact 0 of the same-side product is not close,
it is decided), and no frame may lose more than 2 % of its pixels that way.

MEASURED: the worst |restatement - reference| over the comparable pixels of the 20 frames (what the reference's doubles lose)
is in MEASURED_WORST below, per dimension, specular on / off; BOUND is four times the largest of them -- the factor
test_view_modes.py gives its primary rays over their derived bound, room for a libm that differs by an ulp.
On an MI355X the worst |gpu - restatement| / BOUND per dimension 3 .. 12 was 0.065, 0.056, 0.056, 0.181, 0.081, 0.152, 0.061, 0.118,
0.045, 0.249, and |gpu - reference| 2.7e-15 at worst.

The branch `trace_dist <= EPSILON` of get_ray_color is not in the scene: the intersectors it would have to come from turn away
a hit nearer than EPSILON themselves (hplane.c:60, which the hdisk asks too; sphere.c:87-91; hcylinder.c:201-210), so two flat
objects a fraction of EPSILON apart never produce it.  It is counted (`hit<EPS`: 0 in every fixture) and not required.
The light of the exact tie is a DIRECTIONAL one whose direction lies in the floor's hyperplane, not a point light placed in
it: a floor hit's own coordinate is o + v * d rounded (hplane.c:61-63), a few ulps off the hyperplane, which would make the
sign of a point light's dotRev1 a matter of rounding; -dir . normal is a sum of exact zeros for every hit.

Needs a real MI355X for the tests marked gpu."""
import math
import types

import numpy as np
import pytest

from conftest import golden
from test_shading_paths import DEFAULTS, RENDERS, counts
from test_view_modes import model_rays, need_long_double, _dot, _scale

T = np.longdouble
TOL_TIGHT = 1e-9          # what differing libm ulps can explain (tests/test_gpu_parity.py)
FRAGILE = 1e-9            # a decision nearer than this to its threshold makes its pixel fragile
MAX_FRAGILE = 0.02        # of a frame's pixels: a cap, not a measurement
DIMS = list(range(3, 13))
CELLS = [(d, s) for d in DIMS for s in (1, 0)]
EPS = T(1e-4)             # EPSILON, vectNd.h:25
PI = T(math.pi)           # M_PI: the double
CUT = T(1.0) / T(512.0)
EDGE_DEG = 0.5

# worst |restatement - reference| over the comparable pixels, (specular on, specular off), measured on the CPU
MEASURED_WORST = {
    3: (7.21e-14, 4.08e-14), 4: (6.26e-14, 3.40e-14), 5: (6.26e-14, 6.26e-14), 6: (2.02e-13, 5.65e-14), 7: (8.99e-14, 8.43e-14),
    8: (1.69e-13, 5.77e-14), 9: (6.74e-14, 6.73e-14), 10: (1.31e-13, 4.00e-14), 11: (4.98e-14, 4.59e-14), 12: (2.78e-13, 8.72e-14),
}
BOUND = 4 * 2.78e-13      # 1.112e-12

# branch -> the least number of tree nodes (or light tests of nodes) that take it, per dimension and specular setting
COVERAGE = {
    "tir": 32, "enter": 32, "exit": 32,
    "flip": 32, "noflip": 32,
    "side<0": 32, "side=0": 32,
    "cone_in": 32, "cone_out": 32, "edge_in": 16, "edge_out": 16,
    "by_other": 32, "same_far": 32, "nothing": 32, "dir_lit": 32, "dir_dark": 32,
    "cut_w": 32, "cut_d": 32,
    "refl": 32, "refr": 32, "both": 32,
    "green": 32, "blue": 32, "zero_ch": 32,
    "rv<=0": 32, "rv>0": 32, "max_r": 32, "max_g": 32, "max_b": 32,
}
# (counted but not required: hits within EPSILON of their ray's origin -- see the header)
EXTRA = ("hit<EPS",)


def cell_id(cell):
    return "%dd-spec%d" % cell


# ---------------------------------------------------------------- vectNd.h / vectNd.c in the type of their arguments

def _len(a):
    return np.sqrt(_dot(a, a))


def _unitize(a):
    """vectNd_unitize, vectNd.h:323-329: left alone when no longer than EPSILON.  Returns the vector and |length - EPSILON|."""
    length = _len(a)
    scaled = _scale(a, T(1) / np.where(length > EPS, length, T(1)))
    return np.where((length > EPS)[..., None], scaled, a), np.abs(length - EPS)


def _angle(a, b):
    """vectNd_angle, vectNd.c:64-81."""
    div = _len(a) * _len(b)
    ok = np.abs(div) > EPS
    return np.where(ok, np.arccos(_dot(a, b) / np.where(ok, div, T(1))), T(-1))


def _reflect(u, n, mag):
    """vectNd_reflect, vectNd.c:101-117."""
    return u - _scale(n, (T(1) + T(mag)) * _dot(n, u) / _dot(n, n))


def _refract(u, n, index):
    """vectNd_refract, vectNd.c:119-188.  Returns the direction (not yet unitized), un_dot / |n|, sin_out, and the least margin
    of the two vectNd_unitize calls that could be left undone."""
    rev_u, rev_n = -u, -n
    un_dot = _dot(rev_u, n)
    inside = un_dot < 0
    index = np.where(inside, T(1) / index, index)
    theta_in = np.where(inside, _angle(rev_u, rev_n), _angle(rev_u, n))
    sin_out = np.sin(theta_in) / index
    theta_out = np.where(sin_out <= T(1), np.arcsin(np.minimum(sin_out, T(1))), PI - theta_in)
    rev_n, m1 = _unitize(rev_n)
    n1, _ = _unitize(n)
    un = _scale(rev_n, _dot(u, rev_n))                      # vectNd_proj_unit, vectNd.h:346
    perp, m2 = _unitize(u - un)
    ref_n = _scale(np.where(inside[..., None], n1, rev_n), np.cos(theta_out))
    return ref_n + _scale(perp, np.sin(theta_out)), un_dot / _len(n), sin_out, np.minimum(m1, m2)


# ---------------------------------------------------------------- the scene's shading inputs

class Shading:
    """What apply_lights and get_ray_color read of a scene, in long double."""

    def __init__(self, fs):
        self.fs, self.dims = fs, fs.dims
        self.ambient = np.array(fs.ambient, dtype=T)
        self.background = np.array(fs.background, dtype=T)
        self.lights = []
        for l in fs.lights:
            self.lights.append(types.SimpleNamespace(
                type=l["type"], colour=np.array([l["red"], l["green"], l["blue"]], dtype=T), angle=T(l["angle"]),
                pos=fs.vec(l["pos_off"]).astype(T) if l["pos_off"] >= 0 else None,
                dir=fs.vec(l["dir_off"]).astype(T) if l["dir_off"] >= 0 else None))
        objs = fs.objects
        self.colour = np.array([[o["red"], o["green"], o["blue"]] for o in objs], dtype=T)
        self.refl = np.array([[o["red_r"], o["green_r"], o["blue_r"]] for o in objs], dtype=T)
        self.index = np.array([o["refract_index"] for o in objs], dtype=T)
        self.transparent = np.array([o["transparent"] != 0 for o in objs])


def _trace(oracle, fs, origin, direction, limit):
    """oracle.trace of rays whose origins and directions are rounded to the doubles the tracer takes."""
    n = len(origin)
    rays = np.empty((n, 2 * fs.dims + 1))
    rays[:, :fs.dims] = origin
    rays[:, fs.dims:2 * fs.dims] = direction
    rays[:, 2 * fs.dims] = limit
    obj, hit, nrm = oracle.trace(fs, rays)
    return obj, hit.astype(T), nrm.astype(T)


class Tally:
    def __init__(self, n_pixels):
        self.count = {k: 0 for k in list(COVERAGE) + list(EXTRA)}
        self.fragile = np.zeros(n_pixels, dtype=bool)

    def add(self, key, mask):
        self.count[key] += int(np.count_nonzero(mask))

    def decided(self, pix, margin, exact_is_decided=None):
        """Pixels `pix` made a decision `margin` away from its threshold."""
        close = np.abs(margin) < FRAGILE
        if exact_is_decided is not None:
            close &= ~exact_is_decided
        self.fragile[pix[close]] = True


def apply_lights(sh, oracle, tally, specular, pix, obj, src, look, hit, nrm):
    """apply_lights (ndt.c:71-326) for the hits of one level: their colour before the children are blended in."""
    fs, n = sh.fs, len(obj)
    colour, hitr, transparent = sh.colour[obj], sh.refl[obj], sh.transparent[obj]
    clr = colour * sh.ambient                                                               # ndt.c:89-91
    for l in sh.lights:
        if l.type == 0:                                                                     # LIGHT_AMBIENT, ndt.c:106-111
            clr = clr + colour * l.colour
            continue
        assert l.type in (1, 2, 3)
        directional = l.type == 2
        if directional:
            rev_light, m = _unitize(np.broadcast_to(-l.dir, hit.shape))                     # ndt.c:157-159
        else:
            rev_light, m = _unitize(l.pos - hit)                                            # ndt.c:155
        tally.decided(pix, m)
        rev_view = src - hit
        d1, d2 = _dot(rev_light, nrm), _dot(rev_view, nrm)
        prod = d1 * d2                                                                      # ndt.c:164
        tally.decided(pix, prod / (_len(rev_view) * _len(nrm) ** 2), exact_is_decided=prod == 0)
        tally.add("side<0", prod < 0)
        tally.add("side=0", prod == 0)
        go = prod > 0
        ldist2 = np.ones(n, dtype=T)
        if directional:
            light_vec = np.broadcast_to(l.dir, hit.shape)                                   # ndt.c:252 (not unitized)
            near, m = _unitize(np.broadcast_to(l.dir, hit.shape))
            tally.decided(pix, m)
            s_origin, s_dir, s_limit = hit + near * (-EPS), rev_light, np.zeros(n)          # ndt.c:232-239
        else:
            light_vec = hit - l.pos                                                         # ndt.c:194-197
            ldist2 = _dot(light_vec, light_vec)
            light_vec, m = _unitize(light_vec)
            tally.decided(pix, m)
            if l.type == 3:                                                                 # ndt.c:201-207
                deg = _angle(np.broadcast_to(l.dir, hit.shape), light_vec) * T(180.0) / PI
                outside = deg > l.angle
                tally.decided(pix[go], (deg - l.angle)[go])
                tally.add("cone_in", go & ~outside)
                tally.add("cone_out", go & outside)
                tally.add("edge_in", go & ~outside & (deg > l.angle - T(EDGE_DEG)))
                tally.add("edge_out", go & outside & (deg < l.angle + T(EDGE_DEG)))
                go = go & ~outside
            s_origin = np.broadcast_to(l.pos, hit.shape)
            s_dir = light_vec
            s_limit = (_len(hit - l.pos) + EPS).astype(np.float64)                          # ndt.c:187-188
        idx = np.flatnonzero(go)
        sobj, shit, snrm = _trace(oracle, fs, s_origin[idx], s_dir[idx], s_limit[idx])
        if directional:
            lit = sobj < 0                                                                  # ndt.c:246
            tally.add("dir_lit", lit)
            tally.add("dir_dark", ~lit)
            lhn = nrm[idx]                                                                  # ndt.c:254
        else:
            same = sobj == obj[idx]                                                         # ndt.c:217
            dist = _len(hit[idx] - shit)                                                    # ndt.c:223
            tally.decided(pix[idx][same], (dist - EPS)[same])
            lit = same & ~(dist > EPS)                                                      # ndt.c:225
            tally.add("nothing", sobj < 0)
            tally.add("by_other", (sobj >= 0) & ~same)
            tally.add("same_far", same & (dist > EPS))
            lhn = snrm
        idx, lhn = idx[lit], lhn[lit]
        lv, nm = light_vec[idx], nrm[idx]
        angle = _angle(nm, lv)                                                              # ndt.c:263
        flip = angle > PI / T(2.0)
        tally.decided(pix[idx], angle - PI / T(2.0))
        tally.add("flip", flip)
        tally.add("noflip", ~flip)
        angle = np.where(flip, PI - angle, angle)
        light_scale = np.cos(angle) / ldist2[idx]
        diffuse = _scale(colour[idx] * l.colour, light_scale)                              # ndt.c:270-272
        add = np.where(transparent[idx][:, None], T(0), diffuse)
        light_ref, m = _unitize(_reflect(lv, lhn, 0.5))                                    # ndt.c:289-294
        tally.decided(pix[idx], m)
        rev_look, _ = _unitize(-look[idx])
        rv = _dot(light_ref, rev_look)
        tally.add("rv<=0", rv <= 0)
        tally.add("rv>0", rv > 0)
        tally.add(("max_r", "max_g", "max_b")[int(np.argmax(l.colour))], np.ones(len(idx), dtype=bool))
        if specular:
            rvn = np.power(np.maximum(T(0), rv), T(50))                                     # ndt.c:299-300
            add = add + _scale(hitr[idx] * l.colour / l.colour.max(), rvn)                  # ndt.c:302-305
        clr[idx] = clr[idx] + add
    return clr


def restate(fs, oracle, width, height, depth, specular):
    """get_ray_color (ndt.c:329-450) for every pixel, level by level.  Returns the (height, width, 4) frame in long double, the
    branch counts and the mask of fragile pixels."""
    sh, d = Shading(fs), fs.dims
    view = types.SimpleNamespace(cam=dict(fs.cam, left_eye=fs.cam["pos"], right_eye=fs.cam["pos"]), vec=fs.vec, cam_type=fs.cam_type,
                                 cam_focal_distance=fs.cam_focal_distance, cam_h_fov=fs.cam_h_fov, cam_v_fov=fs.cam_v_fov)
    assert fs.cam_type == 0
    origin, look = model_rays(view, width, height, 0, T)
    n_pixels = width * height
    tally = Tally(n_pixels)
    level = types.SimpleNamespace(pix=np.arange(n_pixels), src=origin.reshape(-1, d), look=look.reshape(-1, d),
                                  frac=np.ones(n_pixels, dtype=T), parent=None, kind=None)
    levels = []
    for depth_left in range(depth, 0, -1):
        lv = level
        n = len(lv.pix)
        obj, hit, nrm = _trace(oracle, fs, lv.src, lv.look, -np.ones(n))                    # ndt.c:357
        trace_dist = _len(hit - lv.src)
        found = obj >= 0
        tally.decided(lv.pix[found], (trace_dist - EPS)[found])
        tally.add("hit<EPS", found & ~(trace_dist > EPS))
        is_hit = found & (trace_dist > EPS)                                                 # ndt.c:376
        lv.colour = np.empty((n, 4), dtype=T)
        lv.colour[:] = sh.background                                                        # ndt.c:438-441
        h = np.flatnonzero(is_hit)
        lv.h = h
        o, pix, hh, nn, ll, frac = obj[h], lv.pix[h], hit[h], nrm[h], lv.look[h], lv.frac[h]
        lv.own = apply_lights(sh, oracle, tally, specular, pix, o, lv.src[h], ll, hh, nn)
        lv.hitr = sh.refl[o]
        contrib = lv.hitr.max(axis=1)                                                       # ndt.c:393
        lv.has_refl = contrib > 0
        lv.has_refr = sh.transparent[o]
        tally.add("refl", lv.has_refl & ~lv.has_refr)
        tally.add("refr", ~lv.has_refl & lv.has_refr)
        tally.add("both", lv.has_refl & lv.has_refr)
        tally.add("green", lv.has_refl & (np.argmax(lv.hitr, axis=1) == 1))
        tally.add("blue", lv.has_refl & (np.argmax(lv.hitr, axis=1) == 2))
        tally.add("zero_ch", lv.has_refl & (lv.hitr == 0).any(axis=1))
        lv.ref = [np.zeros((len(h), 3), dtype=T), np.zeros((len(h), 3), dtype=T)]           # what the children returned: black if cut off
        nxt = types.SimpleNamespace(pix=[], src=[], look=[], frac=[], parent=[], kind=[])
        for kind, has, child_frac in ((0, lv.has_refl, contrib * frac), (1, lv.has_refr, (T(1) - contrib) * frac)):
            tally.decided(pix[has], (child_frac - CUT)[has])
            cut_w = has & (child_frac < CUT)                                                # ndt.c:336
            cut_d = has & ~cut_w & (depth_left - 1 <= 0)                                    # ndt.c:340
            tally.add("cut_w", cut_w)
            tally.add("cut_d", cut_d)
            k = np.flatnonzero(has & ~cut_w & ~cut_d)
            if kind == 0:
                ray = _reflect(ll[k], nn[k], 1.0)                                           # ndt.c:398
            else:
                ray, un_dot, sin_out, m = _refract(ll[k], nn[k], sh.index[o[k]])            # ndt.c:423
                tally.decided(pix[k], m)
                tally.decided(pix[k], un_dot)
                tally.decided(pix[k][un_dot < 0], (sin_out - T(1))[un_dot < 0])
                tally.add("enter", ~(un_dot < 0))
                tally.add("tir", (un_dot < 0) & (sin_out > T(1)))
                tally.add("exit", (un_dot < 0) & ~(sin_out > T(1)))
            ray, m = _unitize(ray)
            tally.decided(pix[k], m)
            nxt.pix.append(pix[k]); nxt.src.append(hh[k]); nxt.look.append(ray); nxt.frac.append(child_frac[k])
            nxt.parent.append(k); nxt.kind.append(np.full(len(k), kind))
        levels.append(lv)
        level = types.SimpleNamespace(**{key: np.concatenate(val) for key, val in vars(nxt).items()})
        if len(level.pix) == 0:
            break
    assert depth_left == 1 or len(level.pix) == 0
    for at in range(len(levels) - 1, -1, -1):                                               # the blend, ndt.c:402-429
        lv = levels[at]
        c = lv.own
        refl, refr = lv.has_refl[:, None], lv.has_refr[:, None]
        if specular:
            c = np.where(refl, (T(1) - lv.hitr) * c + lv.hitr * lv.ref[0], c)
        else:
            c = np.where(refl, c + lv.hitr * lv.ref[0], c)
        c = np.where(refr, c + (T(1.0) - lv.hitr) * lv.ref[1], c)
        lv.colour[lv.h, :3] = c
        lv.colour[lv.h, 3] = T(1)
        if lv.parent is not None:
            up = levels[at - 1]
            for kind in (0, 1):
                sel = lv.kind == kind
                up.ref[kind][lv.parent[sel]] = lv.colour[sel, :3]
    return levels[0].colour.reshape(height, width, 4), tally.count, tally.fragile.reshape(height, width)


_restated = {}


def restated(oracle, dims, specular):
    """(frame, counts, fragile pixels) of a fixture: computed once, shared by the CPU and the GPU tests, never written to."""
    key = (dims, specular)
    if key not in _restated:
        g = golden("shade%dd" % dims)
        frame, count, fragile = restate(g.scene, oracle, g.width, g.height, g.depth, specular)
        frame.setflags(write=False)
        fragile.setflags(write=False)
        _restated[key] = (frame, count, fragile)
    return _restated[key]


def reference_frame(g, specular):
    return g.data["fb" if specular else "fb_nospec"]


def reference_total(g, specular):
    """The trace_kd calls of the reference's render: what rays_ref_equiv restates (every pixel's samples, ndt.c:488)."""
    return g.meta["rays_total" if specular else "rays_total_nospec"]


# ---------------------------------------------------------------- CPU

@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_every_branch_is_taken_and_few_pixels_are_fragile(oracle, cell):
    need_long_double()
    dims, specular = cell
    _, count, fragile = restated(oracle, dims, specular)
    print("%2d-D spec %d  " % cell + " ".join("%s %d" % (k, v) for k, v in count.items()) + "  fragile %d" % fragile.sum())
    short = {k: (count[k], least) for k, least in COVERAGE.items() if count[k] < least}
    assert not short, "branches taken too seldom (taken, least): %r" % short
    assert fragile.mean() <= MAX_FRAGILE, "%d of %d pixels are fragile" % (fragile.sum(), fragile.size)


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_restatement_against_the_reference(oracle, cell):
    need_long_double()
    dims, specular = cell
    frame, _, fragile = restated(oracle, dims, specular)
    want = reference_frame(golden("shade%dd" % dims), specular)
    err = np.abs(frame - want.astype(T))[~fragile]
    print("%2d-D spec %d: max |restatement - reference| %.3g over %d pixels (bound %.3g)" % (dims, specular, float(err.max()), (~fragile).sum(), BOUND))
    assert float(err.max()) <= BOUND


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_oracle_against_the_reference(oracle, cell):
    dims, specular = cell
    g = golden("shade%dd" % dims)
    got, st = oracle.render(g.scene, g.width, g.height, g.depth, specular=specular)
    total = reference_total(g, specular)
    diff = np.abs(got - reference_frame(g, specular)).max()
    print("%2d-D spec %d: max |oracle - reference| %g" % (dims, specular, diff))
    assert diff < TOL_TIGHT
    assert st.rays_ref_equiv == total


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


def render_with(gpu, g, options, depth, specular, row_begin=0, row_step=1):
    """One render of a fixture at its own size under pipeline 1 with `options` on top; the options are back at their defaults
    afterwards."""
    chosen = dict(DEFAULTS, pipeline=1)
    chosen.update(options)
    try:
        for name, value in chosen.items():
            gpu.set_option(name, value)
        gpu.upload_scene(g.scene)
        return gpu.render(g.width, g.height, depth, row_begin=row_begin, row_step=row_step, specular=specular)
    finally:
        for name, value in DEFAULTS.items():
            gpu.set_option(name, value)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_every_shading_caller_against_the_reference_and_the_restatement(gpu, oracle, cell):
    """Pipeline 1, pipeline 2, light_overlap 0 and light windows of two entries and of one: the same bytes and counts, the
    reference's count (a shadow ray fired for the light of the exact tie shows here and nowhere else: it would add about
    cos(pi/2) to the colour), the reference's frame within TOL_TIGHT, the long double frame within BOUND."""
    need_long_double()
    dims, specular = cell
    g = golden("shade%dd" % dims)
    runs = [(what, render_with(gpu, g, options, g.depth, specular)) for what, options in RENDERS]
    first, first_st = runs[0][1]
    for what, (out, st) in runs[1:]:
        print("%2d-D spec %d, %s: %d values differ, counts %s" % (dims, specular, what, int((out != first).sum()), counts(st)))
        assert out.tobytes() == first.tobytes(), what
        assert counts(st) == counts(first_st), what
    _, wst = oracle.render(g.scene, g.width, g.height, g.depth, specular=specular)
    print("%2d-D spec %d: counts %s, the reference's total %d" % (dims, specular, counts(first_st), reference_total(g, specular)))
    assert first_st.rays_ref_equiv == reference_total(g, specular)
    assert counts(first_st)[:4] == (wst.rays_primary, wst.rays_secondary, wst.rays_shadow, wst.rays_ref_equiv)
    diff = np.abs(first - reference_frame(g, specular)).max()
    frame, _, fragile = restated(oracle, dims, specular)
    err = float(np.abs(first.astype(T) - frame)[~fragile].max())
    print("%2d-D spec %d: max |gpu - reference| %.3g, max |gpu - restatement| %.3g = %.3f of the bound" % (dims, specular, diff, err, err / BOUND))
    assert diff < TOL_TIGHT
    assert err <= BOUND


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("dims", [3, 7, 12])
def test_shallow_trees_whose_deepest_bounce_is_blended_elsewhere(gpu, oracle, dims, depth):
    """Depth 1, 2 and 3 (test_shading_paths.py: the deepest bounce is lit and blended by other kernels than the ones between)."""
    g = golden("shade%dd" % dims)
    for specular in (1, 0):
        out, st = render_with(gpu, g, {}, depth, specular)
        want, wst = oracle.render(g.scene, g.width, g.height, depth, specular=specular)
        diff = np.abs(out - want).max()
        print("%2d-D depth %d spec %d: max |gpu - oracle| %g, counts %s" % (dims, depth, specular, diff, counts(st)))
        assert diff < TOL_TIGHT
        assert counts(st)[:4] == (wst.rays_primary, wst.rays_secondary, wst.rays_shadow, wst.rays_ref_equiv)


@pytest.mark.gpu
def test_row_shards_of_the_12d_frame(gpu):
    g = golden("shade12d")
    full, _ = render_with(gpu, g, {}, g.depth, 1)
    for begin in range(3):
        part, _ = render_with(gpu, g, {}, g.depth, 1, row_begin=begin, row_step=3)
        assert part.tobytes() == full[begin::3].tobytes(), "rows %d, %d, ..." % (begin, begin + 3)

"""The stochastic half of the renderer, value for value ("The stream contract").

`-n samples` > 1, depth of field and LIGHT_DISK / LIGHT_RECT draw from counter-based streams on the device: every number is
uniform(key, k) of a key that depends only on the image position, the sample number, sample_seed + the eye's salt, the path
of reflected / refracted children and the light's place in the list.  The oracle's mode 1 (ndt_oracle_set_streams) draws
exactly those numbers, so every stochastic render has ONE right answer and the device is held to it at the tolerance of the
deterministic tests -- no pixel left out, sample totals equal, depth maps equal.  (The statistical tests of
test_gpu_parity.py stay: they test another claim, agreement with the reference's own drand48 stream.)

What lets a tolerance of 1e-9 ask for equality everywhere: a last-bit difference in a colour (ocml against glibc behind a
refraction) could flip an adaptive loop's exit or a subdivision only if the tested value sat on its threshold.  The oracle
reports the smallest distance of any such decision from its threshold; the sample_seeds below were chosen, on the CPU, so
that it is >= 1e-6 for every case, and the CPU part of this file asserts it.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import comparable, golden, SAMPLED_CASES, SAMPLED_MODE_CASES

TOL_TIGHT = 1e-9        # the deterministic tests' tolerance (test_gpu_parity.py): what differing libm ulps can explain
MARGIN = 1e-6           # every loop / subdivision decision lies at least this far from its threshold
DRAWS = ["jitter", "lens", "lens_reject", "lens_cap", "disk", "disk_reject", "disk_cap", "rect", "area_primary", "area_reflected",
         "area_refracted"]
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the oracle's replay mode

def replay_lib(oracle):
    lib = oracle.lib
    if getattr(lib, "_replay_ready", False):
        return lib
    u64 = C.c_ulonglong
    lib.ndt_oracle_set_streams.argtypes = [C.c_int, u64]
    lib.ndt_oracle_set_streams.restype = None
    lib.ndt_oracle_replay_samples.restype = C.c_longlong
    lib.ndt_oracle_replay_margin.restype = C.c_double
    lib.ndt_oracle_replay_aa_margin.restype = C.c_double
    lib.ndt_oracle_replay_draws.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    lib.ndt_oracle_replay_draws.restype = C.c_int
    lib.ndt_oracle_stream_mix.argtypes = [u64]
    lib.ndt_oracle_stream_mix.restype = u64
    lib.ndt_oracle_stream_uniform.argtypes = [u64, C.c_uint]
    lib.ndt_oracle_stream_uniform.restype = C.c_double
    lib.ndt_oracle_stream_sample_key.argtypes = [u64, C.c_uint, u64]
    lib.ndt_oracle_stream_sample_key.restype = u64
    lib.ndt_oracle_stream_list_id.argtypes = [C.c_double, C.c_double]
    lib.ndt_oracle_stream_list_id.restype = u64
    lib.ndt_oracle_stream_child_key.argtypes = [u64, C.c_int]
    lib.ndt_oracle_stream_child_key.restype = u64
    lib.ndt_oracle_stream_lens.argtypes = [u64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ndt_oracle_stream_lens.restype = C.c_int
    lib.ndt_oracle_stream_light.argtypes = [u64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.ndt_oracle_stream_light.restype = C.c_int
    lib._replay_ready = True
    return lib


class Replayed:
    """One mode-1 oracle render and what it reports."""

    def __init__(self, img, depth, st, lib):
        self.img, self.depth, self.st = img, depth, st
        self.samples = int(lib.ndt_oracle_replay_samples())
        self.margin = float(lib.ndt_oracle_replay_margin())
        self.aa_margin = float(lib.ndt_oracle_replay_aa_margin())
        d = (C.c_longlong * len(DRAWS))()
        assert lib.ndt_oracle_replay_draws(d, len(DRAWS)) == len(DRAWS)
        self.draws = dict(zip(DRAWS, [int(v) for v in d]))

    def report(self):
        return "samples %d, decision margin %.3g%s, draws %s" % (
            self.samples, self.margin, "" if self.aa_margin > 1e300 else ", subdivision margin %.3g" % self.aa_margin,
            " ".join("%s=%d" % (k, v) for k, v in self.draws.items() if v))


def replay(oracle, fs, w, h, depth, seed, **kw):
    """The oracle's render of the device's streams for sample_seed `seed` (mode 1), on the oracle's threads."""
    lib = replay_lib(oracle)
    want_depth = kw.get("depth_map", False)
    lib.ndt_oracle_set_streams(1, seed)
    try:
        r = oracle.render(fs, w, h, depth, **kw)
        return Replayed(r[0], r[1] if want_depth else None, r[-1], lib)
    finally:
        lib.ndt_oracle_set_streams(0, 0)


# ---------------------------------------------------------------- scenes

def fresh(name):
    """A copy of a fixture's scene of its own (golden() shares its scene)."""
    from ndt_amd.flat_scene import FlatScene
    src, fs = golden(name).scene, FlatScene()
    for key, value in src.__dict__.items():
        if key == "lights":
            fs.lights = [dict(l) for l in value]
        elif isinstance(value, (list, dict)):
            setattr(fs, key, type(value)(value))        # (objects and kd nodes are shared: nothing here edits them)
        elif not isinstance(value, np.ndarray) and not hasattr(value, "_b_base_") and not hasattr(value, "_fields_"):
            setattr(fs, key, value)
    fs._struct = None
    return fs.finalize()


def _unit(v):
    return v / np.sqrt((v * v).sum())


def orthonormal_pair(d, seed, away_from=()):
    """Two orthonormal d-vectors with every component in use, orthogonal to the vectors of `away_from`."""
    rng = np.random.default_rng(seed)
    basis = [_unit(np.asarray(a, dtype=np.float64)) for a in away_from]
    out = []
    while len(out) < 2:
        v = rng.uniform(-1.0, 1.0, d)
        for b in basis + out:
            v = v - (v * b).sum() * b
        out.append(_unit(v))
    return out


def give_lens(fs, aperture):
    """An aperture; an `ndtscene 1` file has no local axes: two unit vectors orthogonal to the view direction and to each
    other (both sides read the same vectors, which is all the replay needs)."""
    fs.cam_aperture_radius = aperture
    if "local_x" not in fs.cam or "local_y" not in fs.cam:
        view = fs.vec(fs.cam["img_orig"]) - fs.vec(fs.cam["pos"])
        lx, ly = orthonormal_pair(fs.dims, 11, away_from=[view])
        fs.cam["local_x"] = fs.add_vec(list(lx))
        fs.cam["local_y"] = fs.add_vec(list(ly))
        fs.cam.setdefault("local_z", fs.add_vec(list(_unit(view))))     # (the device asks for all three; a planar camera reads two)
    fs._struct = None
    fs.finalize()
    return fs


def stochastic_zoo(name, aperture=0.08, radius=0.3):
    """A deterministic fixture made stochastic in every way at once: its first point light becomes a LIGHT_DISK, a LIGHT_RECT
    is appended next to it, and the camera gets an aperture."""
    fs = fresh(name)
    d = fs.dims
    k = next(i for i, l in enumerate(fs.lights) if l["type"] == 1)
    disk = fs.lights[k]
    u, v = orthonormal_pair(d, 100 + d)
    disk["type"], disk["radius"] = 4, radius
    disk["area_off"] = fs.add_vec(list(u))
    fs.add_vec(list(v))
    u2, v2 = orthonormal_pair(d, 200 + d)
    shift = np.zeros(d)
    shift[0], shift[d - 1] = 0.7, -0.4
    rect = dict(type=5, red=0.5 * disk["red"], green=0.6 * disk["green"], blue=0.4 * disk["blue"], angle=0.0,
                pos_off=fs.add_vec(list(fs.vec(disk["pos_off"]) + shift)), dir_off=-1, radius=1.1 * radius)
    rect["area_off"] = fs.add_vec(list(u2))
    fs.add_vec(list(v2))
    disk["red"], disk["green"], disk["blue"] = 0.6 * disk["red"], 0.6 * disk["green"], 0.6 * disk["blue"]
    fs.lights.append(rect)
    return give_lens(fs, aperture)


def many_lights_with_area(n_total):
    """al_zoo4d with its list grown past one window of lights (test_many_lights.py) and area lights at list positions 0, 63,
    64 and the last: the draw of a light is keyed by its place in the LIST, whichever window shades it."""
    from test_many_lights import with_many_lights
    fs = with_many_lights(fresh("al_zoo4d"), n_total)
    d = fs.dims
    own = [dict(l) for l in fs.lights if l["type"] in (4, 5)]
    assert own, "al_zoo4d has area lights"
    for n, at in enumerate((0, 63, 64, n_total - 1)):
        src = own[n % len(own)]
        u, v = orthonormal_pair(d, 300 + at)
        shift = np.zeros(d)
        shift[n % d] = 0.5 + 0.25 * n
        l = dict(src, type=4 + n % 2, red=0.3 * src["red"], green=0.3 * src["green"], blue=0.3 * src["blue"],
                 pos_off=fs.add_vec(list(fs.vec(src["pos_off"]) + shift)), radius=0.3 + 0.05 * n)
        l["area_off"] = fs.add_vec(list(u))
        fs.add_vec(list(v))
        fs.lights[at] = l
    fs._struct = None
    fs.finalize()
    return fs


_scenes = {}


def scene(key):
    """Scenes by name: "zoo:<fixture>" (stochastic_zoo), "lens:<fixture>" (the fixture with an aperture), "lights:<n>", or a
    fixture's own."""
    if key not in _scenes:
        kind, _, arg = key.partition(":")
        if kind == "zoo":
            _scenes[key] = stochastic_zoo(arg)
        elif kind == "lens":
            _scenes[key] = give_lens(fresh(arg), 0.25 if arg == "c1_hypercube3d" else 0.08)
        elif kind == "lights":
            _scenes[key] = many_lights_with_area(int(arg))
        else:
            _scenes[key] = golden(key).scene
    return _scenes[key]


# ---------------------------------------------------------------- cases

class Case:
    def __init__(self, cid, scene_key, w, h, depth, S, seeds, stereo=0, depth_map=False, rows=(0, 1), aa=None):
        self.id, self.scene_key, self.w, self.h, self.depth, self.S, self.seeds = cid, scene_key, w, h, depth, S, seeds
        self.stereo, self.depth_map, self.rows, self.aa = stereo, depth_map, rows, aa

    def kw(self):
        kw = dict(row_begin=self.rows[0], row_step=self.rows[1], stereo=self.stereo, samples=self.S)
        if self.aa is not None:
            kw["aa"] = self.aa
        if self.depth_map:
            kw["depth_map"] = True
        return kw


ZOO = {3: "zoo3d_mirror", 4: "zoo4d", 5: "zoo5d_f2", 6: "zoo6d", 7: "zoo7d", 8: "zoo8d", 9: "zoo9d", 10: "zoo10d", 11: "zoo11d",
       12: "zoo12d"}
# sample_seeds: two per case, chosen on the CPU so that the case's decision margins are >= MARGIN (test_replay_case_*
# asserts it); a case that is not listed takes DEFAULT_SEEDS
DEFAULT_SEEDS = (103, 106)
SEEDS = {
    "ns_zoo4d_dof-S2": (141, 171), "ns_zoo4d_dof-S5": (141, 171),
    "al_zoo4d-S2": (228, 440), "al_zoo4d-S5": (228, 440),
    "al_zoo3d_dof_n3-S2": (163, 173), "al_zoo3d_dof_n3-S5": (163, 173),
    "ns_zoo4d_sbs-S2": (107, 154), "ns_zoo4d_sbs-S5": (107, 154),
    "ns_vr_zoo4d-S2": (102, 106), "ns_vr_zoo4d-S5": (102, 106),
    "ns_zoo3d_anaglyph-S2": (322, 426), "ns_zoo3d_anaglyph-S5": (322, 426),
    "ns_zoo3d_hidef-S2": (108, 181), "ns_zoo3d_hidef-S5": (108, 181),
    "al_zoo4d-S1": (101, 121), "al_zoo3d_dof_n3-S1": (103, 117),
    "zoo3d-S3": (101, 102), "zoo4d-S3": (106, 108), "zoo5d-S3": (102, 117), "zoo6d-S3": (140, 169), "zoo7d-S3": (108, 109),
    "zoo8d-S3": (105, 106), "zoo9d-S3": (101, 106), "zoo10d-S3": (101, 103), "zoo11d-S3": (101, 103), "zoo12d-S3": (102, 103),
    "lights70-S2": (102, 106),
    "zoo4d-S1": (101, 102), "zoo4d-S2": (106, 108), "zoo4d-S9": (106, 108), "zoo4d-S70": (101, 102),
    "c1_hypercube3d-lens-320x216": (361, 395),
    "aa-aa_zoo4d_dof": (1003, 5397), "aa-al_zoo4d": (1187, 1041), "aa-anaglyph-lens": (32, 139),
}


def _seeds(cid):
    return SEEDS.get(cid, DEFAULT_SEEDS)


def _fixture_cases():
    out = []
    for name in SAMPLED_CASES + SAMPLED_MODE_CASES:
        g = golden(name)
        stereo = g.meta.get("stereo", 0)
        # the frame-packed image: a row shard over lines 1070 .. 2200 in steps of 5 -- the left eye's last lines, every fifth
        # blank line with both ends of the band (1080, 1125), the right eye
        rows = (1070, 5) if stereo == 4 else (0, 1)
        for S in (2, 5):
            cid = "%s-S%d" % (name, S)
            out.append(Case(cid, name, g.width, g.height, g.depth, S, _seeds(cid), stereo=stereo, depth_map="depth" in g.data,
                            rows=rows))
    for name in ("al_zoo4d", "al_zoo3d_dof_n3"):       # the area lights alone drive the loop
        g = golden(name)
        cid = "%s-S1" % name
        out.append(Case(cid, name, g.width, g.height, g.depth, 1, _seeds(cid)))
    return out


FIXTURE_CASES = _fixture_cases()
DIM_CASES = [Case("zoo%dd-S3" % d, "zoo:" + ZOO[d], 16, 9, 4, 3, _seeds("zoo%dd-S3" % d)) for d in range(3, 13)]
LIGHT_CASES = [Case("lights70-S2", "lights:70", 16, 9, 3, 2, _seeds("lights70-S2"))]
SHARD_CASES = [Case("zoo4d-S3-rows%d/%d" % r, "zoo:zoo4d", 16, 9, 4, 3, _seeds("zoo4d-S3"), rows=r) for r in ((1, 2), (2, 3))]
# (the anaglyph runs two loops per anti-aliasing sample: at aa_depth 2 none of 6 000 sample_seeds kept all of its ~1.4 M loop
# decisions 1e-6 clear of the threshold, at aa_depth 1 about one in a hundred does)
AA_CASES = [Case("aa-aa_zoo4d_dof", "aa_zoo4d_dof", 16, 9, 4, 1, _seeds("aa-aa_zoo4d_dof"), aa=(20, 2)),
            Case("aa-al_zoo4d", "al_zoo4d", 16, 9, 4, 1, _seeds("aa-al_zoo4d"), aa=(20, 2)),
            Case("aa-anaglyph-lens", "lens:aa_zoo3d_anaglyph", 16, 9, 4, 1, _seeds("aa-anaglyph-lens"), stereo=3, aa=(20, 1))]
COUNT_CASES = [Case("zoo4d-S%d" % S, "zoo:zoo4d", 16, 9, 4, S, _seeds("zoo4d-S%d" % S)) for S in (1, 2, 9, 70)]
# more than 65 536 active pixels: per_pass / n_active limits the samples a pass renders ahead
BIG_CASE = Case("c1_hypercube3d-lens-320x216", "lens:c1_hypercube3d", 320, 216, 2, 2, _seeds("c1_hypercube3d-lens-320x216"))
ALL_CASES = FIXTURE_CASES + DIM_CASES + LIGHT_CASES + SHARD_CASES + AA_CASES + COUNT_CASES + [BIG_CASE]

_replays = {}


def replayed(oracle, case, seed):
    """The oracle's answer for (case, seed): computed once, shared, never written to."""
    key = (case.id, seed)
    if key not in _replays:
        r = replay(oracle, scene(case.scene_key), case.w, case.h, case.depth, seed, **case.kw())
        r.img.setflags(write=False)
        if r.depth is not None:
            r.depth.setflags(write=False)
        _replays[key] = r
    return _replays[key]


# ---------------------------------------------------------------- CPU: the contract, restated once more with numpy integers

def np_mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9e3779b97f4a7c15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def np_uniform(key, k):
    with np.errstate(over="ignore"):
        h = np_mix(np.asarray(key, dtype=np.uint64) + np.uint64(k))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def np_sample_key(pid, rnd, seed):
    with np.errstate(over="ignore"):
        key = np_mix(np.asarray(pid, dtype=np.uint64) * np.uint64(0x100000001b3) + np.uint64(rnd))
        if seed != 0:
            key = key ^ np_mix(np.uint64(seed) * np.uint64(0x9e3779b97f4a7c15) + np.uint64(0x632be59bd9b4e019))
    return key


def np_list_id(i, j):
    bi = np.asarray(i, dtype=np.float64).view(np.uint64)
    bj = np.asarray(j, dtype=np.float64).view(np.uint64)
    with np.errstate(over="ignore"):
        return np_mix(bi) ^ np_mix(bj + np.uint64(0x7f4a7c159e3779b9))


def np_rejection(key, first, last, reject):
    """Pairs 2u - 1 at indices first, first + 1, then + 2 per rejected try; the try at `last` is kept whatever it is."""
    k, tries = first, 0
    while True:
        x, y = 2 * float(np_uniform(key, k)) - 1.0, 2 * float(np_uniform(key, k + 1)) - 1.0
        tries += 1
        if not (reject and x * x + y * y > 1.0) or k >= last:
            return x, y, tries
        k += 2


def np_light_key(node, li):
    with np.errstate(over="ignore"):
        return np_mix(np.asarray(node, dtype=np.uint64) ^ (np.uint64(0x51ed270b27b4f3cf) * np.uint64(li + 1)))


def test_mix_is_splitmix64():
    """splitmix64's published vector: state 1234567 gives 6457827717110365317, then 3203168211198807973.  mix(z) is the
    generator's output for the state z (it adds the increment itself)."""
    inc = 0x9e3779b97f4a7c15
    assert int(np_mix(1234567)) == 6457827717110365317
    assert int(np_mix((1234567 + inc) & M64)) == 3203168211198807973


def test_oracle_mix_and_uniform(oracle):
    lib = replay_lib(oracle)
    inc = 0x9e3779b97f4a7c15
    assert lib.ndt_oracle_stream_mix(1234567) == 6457827717110365317
    assert lib.ndt_oracle_stream_mix((1234567 + inc) & M64) == 3203168211198807973
    # [0, 1): the all-ones hash gives the largest value, (2^53 - 1) * 2^-53
    assert ((M64 >> 11) * 2.0 ** -53) == 1.0 - 2.0 ** -53 < 1.0
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 63, 4000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 4000, dtype=np.uint64)
    u = np.array([lib.ndt_oracle_stream_uniform(int(k), 7) for k in keys])
    assert (u >= 0.0).all() and (u < 1.0).all()
    assert np.array_equal(u, np_uniform(keys, 7))
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size)


def test_numpy_restatement_agrees_with_the_oracle(oracle):
    """Every row of the contract's table, restated with numpy integers here, against the oracle's C."""
    lib = replay_lib(oracle)
    rng = np.random.default_rng(9)
    big = [int(v) for v in rng.integers(0, 1 << 62, 300, dtype=np.uint64) * np.uint64(4) + np.uint64(3)]
    for n, key in enumerate(big):
        assert lib.ndt_oracle_stream_mix(key) == int(np_mix(key))
        for seed in (0, 1, 20261, 0x5eed0000000000ff, (20261 + 0x5eed0000000000ff) & M64):
            assert lib.ndt_oracle_stream_sample_key(key, n, seed) == int(np_sample_key(key, n, seed))
        for kind in (1, 2):
            assert lib.ndt_oracle_stream_child_key(key, kind) == int(np_mix(key ^ kind))
    # pixel ids are small integers; list ids come from the positions' two doubles
    for pid in (0, 1, 31, 32 * 18 - 1, 12 * 2205 - 1, 320 * 216 - 1):
        for rnd in (0, 1, 2, 69, 9999):
            assert lib.ndt_oracle_stream_sample_key(pid, rnd, 0) == int(np_sample_key(pid, rnd, 0))
    for i, j in ((0.0, 0.0), (3.5, 2.0), (3.0, 2.5), (16.0, 9.0), (7.25, 8.75), (2.5, 3.0), (3.0, 2.5)):
        assert lib.ndt_oracle_stream_list_id(i, j) == int(np_list_id(i, j))
    assert int(np_list_id(2.5, 3.0)) != int(np_list_id(3.0, 2.5))       # the two coordinates are told apart
    ax, ay = C.c_double(), C.c_double()
    lens_tries, disk_tries = [], []
    for key in big:
        t = lib.ndt_oracle_stream_lens(key, C.byref(ax), C.byref(ay))
        assert (ax.value, ay.value, t) == np_rejection(np.uint64(key), 1002, 1062, True)
        lens_tries.append(t)
        for li in (0, 1, 63, 64, 1023):
            t = lib.ndt_oracle_stream_light(key, li, 1, C.byref(ax), C.byref(ay))
            assert (ax.value, ay.value, t) == np_rejection(np_light_key(key, li), 0, 62, True)
            disk_tries.append(t)
            t = lib.ndt_oracle_stream_light(key, li, 0, C.byref(ax), C.byref(ay))
            assert (ax.value, ay.value, t) == np_rejection(np_light_key(key, li), 0, 62, False) and t == 1
    # rejection happens (1 - pi/4 of the tries), more than once in a row too
    assert max(lens_tries) >= 3 and max(disk_tries) >= 3
    assert abs(np.mean(np.array(lens_tries) == 1) - np.pi / 4) < 0.1


def _mode0_ensemble(oracle, g, S, n):
    s0 = g.meta["seed48"]
    return np.array([oracle.render(g.scene, g.width, g.height, g.depth, samples=S, seed48=[(s0[0] + 7919 * k) & 0xffff, s0[1], s0[2]],
                                   stereo=g.meta.get("stereo", 0))[0] for k in range(n)])


@pytest.mark.parametrize("name", ["ns_zoo4d_dof", "al_zoo4d"])
def test_replay_is_one_more_sampler_of_the_same_distribution(oracle, name):
    """Mode 1 against mode 0 (= the reference's drand48 stream), with the statistic and the thresholds
    test_jittered_samples_statistically_match_the_oracle holds the device to: the contract itself is unbiased, and the
    replay is wired to the jitter, the lens and the area lights (a site left on drand48, or fed a constant, shows here)."""
    g = golden(name)
    S, n_seeds, n_dev = 8, 24, 12
    ens = _mode0_ensemble(oracle, g, S, n_seeds)
    dev = np.array([replay(oracle, g.scene, g.width, g.height, g.depth, 1000 + k, samples=S).img for k in range(n_dev)])
    out = dev[0]
    mu, sd = ens.mean(axis=0), ens.std(axis=0, ddof=1)
    noisy = sd > 1e-12
    moved = np.abs(out - mu)[~noisy] >= 1e-9
    assert moved.sum() <= 0.003 * moved.size + 1, (int(moved.sum()), moved.size)
    z = (out - mu)[noisy] / (sd[noisy] * np.sqrt(1.0 + 1.0 / n_seeds))
    frac5 = float((np.abs(z) < 5).mean())
    print("%s S=%d: %d noisy values, mean z %+.3f (|z| clipped at 15; %d beyond), %.2f %% |z|<5" % (
        name, S, int(noisy.sum()), np.clip(z, -15, 15).mean(), int((np.abs(z) >= 15).sum()), 100 * frac5))
    assert (np.abs(z) >= 15).sum() <= 0.005 * z.size
    assert abs(np.clip(z, -15, 15).mean()) < 0.15
    assert frac5 > 0.99
    means = ens[..., :3].mean(axis=(1, 2, 3))
    t = (out[..., :3].mean() - means.mean()) / (means.std(ddof=1) * np.sqrt(1.0 + 1.0 / n_seeds))
    assert abs(t) < 4.5, t
    assert abs(out[..., :3].mean() - means.mean()) < 0.002
    se = np.sqrt(ens.var(axis=0, ddof=1) / n_seeds + dev.var(axis=0, ddof=1) / n_dev)
    both = se > 1e-12
    t2 = np.clip((dev.mean(axis=0) - mu)[both] / se[both], -15, 15)
    print("%s S=%d: mode-1 ensemble (%d) against mode-0 ensemble (%d): per-value t mean %+.3f (unbiased: 0 +- %.3f), rms %.2f" % (
        name, S, n_dev, n_seeds, t2.mean(), 1 / np.sqrt(t2.size), np.sqrt((t2 ** 2).mean())))
    assert abs(t2.mean()) < 4.5 / np.sqrt(t2.size / 3.0), t2.mean()
    assert np.sqrt((t2 ** 2).mean()) < 1.35
    dm = dev[..., :3].mean(axis=(1, 2, 3))
    t_img = (dm.mean() - means.mean()) / np.sqrt(means.var(ddof=1) / n_seeds + dm.var(ddof=1) / n_dev)
    assert abs(t_img) < 4.5, t_img


def test_replay_does_not_depend_on_threads_or_shards(oracle):
    """In mode 1 nothing depends on order: one thread or eight, the whole frame or a row shard."""
    case = DIM_CASES[1]
    fs = scene(case.scene_key)
    a = replay(oracle, fs, case.w, case.h, case.depth, 5, samples=3, threads=1)
    b = replay(oracle, fs, case.w, case.h, case.depth, 5, samples=3, threads=8)
    assert np.array_equal(a.img, b.img) and (a.samples, a.margin, a.draws) == (b.samples, b.margin, b.draws)
    part = replay(oracle, fs, case.w, case.h, case.depth, 5, samples=3, row_begin=1, row_step=2)
    assert np.array_equal(part.img, a.img[1::2])
    other = replay(oracle, fs, case.w, case.h, case.depth, 6, samples=3)
    assert not np.array_equal(other.img, a.img)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_replay_case_decisions_are_clear_of_their_thresholds(oracle, case):
    """The precondition of the GPU tests: no continuation decision of an adaptive loop, and no subdivision decision of the
    anti-aliasing, within MARGIN of its threshold -- a last-bit difference in a colour cannot then change a sample count."""
    for seed in case.seeds:
        r = replayed(oracle, case, seed)
        print("%s seed %d: %s" % (case.id, seed, r.report()))
        assert r.margin >= MARGIN, (case.id, seed, r.margin)
        if case.aa is not None:
            assert r.aa_margin >= MARGIN, (case.id, seed, r.aa_margin)
            assert r.st.pixels_resampled > 0
        assert r.samples >= max(case.S, 1) * 1


@pytest.mark.parametrize("case", DIM_CASES, ids=lambda c: c.id)
def test_dimension_cases_reach_every_kind_of_draw(oracle, case):
    """Before a dimension's case is relied on: the replay takes a reflected child and a refracted child that reach an
    area-light draw, rejects a disk draw and rejects a lens draw."""
    for seed in case.seeds:
        d = replayed(oracle, case, seed).draws
        assert d["jitter"] > 0 and d["lens"] == d["jitter"]
        assert d["area_primary"] > 0 and d["area_reflected"] > 0 and d["area_refracted"] > 0, d
        assert d["disk"] > 0 and d["rect"] > 0 and d["disk_reject"] > 0 and d["lens_reject"] > 0, d


# ---------------------------------------------------------------- GPU: the device against the replay

@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    for name in ("sample_seed", "pipeline", "light_window"):
        ctx.set_option(name, 0)
    ctx.set_option("stream_fused", 1)
    ctx.close()


def device_render(gpu, case, seed):
    gpu.set_option("sample_seed", seed)
    try:
        r = gpu.render(case.w, case.h, case.depth, **case.kw())
    finally:
        gpu.set_option("sample_seed", 0)
    return r[0], (r[1] if case.depth_map else None), r[-1]


def expected_aa_samples(case, want):
    """stats.aa_samples of the device: the samples its adaptive loops consumed; under -a the five samples of every subdivision,
    like the oracle's own aa_samples (the loops inside those samples are not reported there: the image, a mean over exactly
    the consumed samples, is what holds them)."""
    return want.st.aa_samples if case.aa is not None else want.samples


def hold_to_replay(gpu, oracle, case, what=""):
    """(a) the image at TOL_TIGHT over rgba with no mask, (b) the consumed samples exactly, (c) the depth map at TOL_TIGHT,
    (d) for two sample_seeds, which give different images.  Returns the device's images."""
    imgs = []
    for seed in case.seeds:
        want = replayed(oracle, case, seed)
        assert want.margin >= MARGIN
        out, dm, st = device_render(gpu, case, seed)
        diff = np.abs(comparable_rows(out, case) - comparable_rows(want.img, case)).max()
        print("%s%s seed %d: max |device - oracle| %.3g, aa_samples device %d oracle %d; oracle: %s" % (
            case.id, what, seed, diff, st.aa_samples, expected_aa_samples(case, want), want.report()))
        assert diff < TOL_TIGHT, (case.id, what, seed, diff)
        assert st.aa_samples == expected_aa_samples(case, want), (case.id, what, seed)
        if case.aa is not None:
            assert st.pixels_resampled == want.st.pixels_resampled
        if case.depth_map:
            assert np.abs(dm - want.depth).max() < TOL_TIGHT, (case.id, what, seed)
            assert (want.depth > 0).any()
        imgs.append(out)
    assert not np.array_equal(imgs[0], imgs[1]), "two sample_seeds, one image: the streams are not in use"
    assert not np.array_equal(replayed(oracle, case, case.seeds[0]).img, replayed(oracle, case, case.seeds[1]).img)
    return imgs


def comparable_rows(fb, case):
    """conftest.comparable for a row shard: the alpha of the frame-packed image's blank lines is the only value left out."""
    if case.stereo != 4:
        return fb
    full = np.zeros((case.h,) + fb.shape[1:])
    full[case.rows[0]::case.rows[1]] = fb
    return comparable(full, 4)[case.rows[0]::case.rows[1]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIXTURE_CASES, ids=lambda c: c.id)
def test_stochastic_fixtures_value_for_value(gpu, oracle, case):
    """Every stochastic fixture -- jitter, lens, area lights, side by side, VR, anaglyph, frame-packed, depth map -- at S = 2
    and S = 5 (and S = 1 where area lights alone drive the loop)."""
    gpu.upload_scene(scene(case.scene_key))
    hold_to_replay(gpu, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", DIM_CASES, ids=lambda c: c.id)
def test_every_dimension_under_every_pipeline(gpu, oracle, case):
    """N = 3 .. 12: the key hand-down and the area-light draw of both copies of the `template <int N>` code (per-bounce
    kernels, streaming kernel fused and not) against the replay, and against each other bit for bit."""
    gpu.upload_scene(scene(case.scene_key))
    runs = []
    try:
        for pipeline, fused in ((1, 1), (2, 0), (2, 1)):
            gpu.set_option("pipeline", pipeline)
            gpu.set_option("stream_fused", fused)
            runs.append(hold_to_replay(gpu, oracle, case, " pipeline %d stream_fused %d" % (pipeline, fused)))
    finally:
        gpu.set_option("pipeline", 0)
        gpu.set_option("stream_fused", 1)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LIGHT_CASES, ids=lambda c: c.id)
def test_area_lights_in_every_light_window(gpu, oracle, case):
    """More than 64 lights, area lights at list positions 0, 63, 64 and the last, under windows of 64 (the default), 1 and 64
    asked for: a light's draw is keyed by its place in the list (li_base + li)."""
    fs = scene(case.scene_key)
    assert len(fs.lights) > 64 and all(fs.lights[at]["type"] in (4, 5) for at in (0, 63, 64, len(fs.lights) - 1))
    try:
        for lw in (0, 1, 64):
            gpu.set_option("light_window", lw)
            gpu.upload_scene(fs)
            hold_to_replay(gpu, oracle, case, " light_window %d" % lw)
    finally:
        gpu.set_option("light_window", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHARD_CASES, ids=lambda c: c.id)
def test_row_shards_of_a_stochastic_frame(gpu, oracle, case):
    """A row shard equals the oracle's shard and the matching rows of the whole frame."""
    gpu.upload_scene(scene(case.scene_key))
    parts = hold_to_replay(gpu, oracle, case)
    whole = DIM_CASES[1]
    assert whole.scene_key == case.scene_key and whole.seeds == case.seeds
    for part, seed in zip(parts, case.seeds):
        full, _, _ = device_render(gpu, whole, seed)
        assert np.array_equal(part, full[case.rows[0]::case.rows[1]])
        assert np.array_equal(replayed(oracle, case, seed).img, replayed(oracle, whole, seed).img[case.rows[0]::case.rows[1]])


@pytest.mark.gpu
@pytest.mark.parametrize("case", AA_CASES, ids=lambda c: c.id)
def test_recursive_antialiasing_over_the_streams(gpu, oracle, case):
    """-a over the streams: every anti-aliasing sample is an adaptive loop keyed by its position's two doubles (exact dyadic
    fractions on both sides); the eyes of an anaglyph take their salts in list mode too."""
    gpu.upload_scene(scene(case.scene_key))
    for seed in case.seeds:
        assert replayed(oracle, case, seed).aa_margin >= MARGIN
    hold_to_replay(gpu, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", COUNT_CASES, ids=lambda c: c.id)
def test_sample_counts_below_and_above_the_pass_cap(gpu, oracle, case):
    """S = 1, 2, 9 and 70 (above the 64 samples a pass renders at most): the loop consumes the samples one by one and drops
    what was rendered past its exit."""
    gpu.upload_scene(scene(case.scene_key))
    hold_to_replay(gpu, oracle, case)


@pytest.mark.gpu
def test_speculation_on_a_large_frame(gpu, oracle):
    """More than 65 536 active pixels: per_pass / n_active limits what a pass renders ahead in the first rounds after
    `samples`.

    What this case found when it was written: k_ns_samples jittered the pixel's NUMBER (i + dx, rounded at the magnitude of
    i) where the reference jitters x (orig_x + dx / width, ndt.c:505-514), up to 1e-16 apart.  c1_hypercube3d has coincident
    surfaces along its edges; about one sample in 10^5 lands where that picks the other one, and under sample_seed 361 five
    pixels came out up to 0.0385 apart with 8 more samples consumed (device 629444, oracle 629436), under every pipeline and
    in every row shard.  primary_node now adds the jitter to x and y the reference's way."""
    case = BIG_CASE
    assert case.w * case.h > 65536
    gpu.upload_scene(scene(case.scene_key))
    hold_to_replay(gpu, oracle, case)
    want = replayed(oracle, case, case.seeds[0])
    assert want.samples > case.S * case.w * case.h          # the loop went on somewhere

"""The coordinate ladder: every float a reprojection can hand the lookup kernels, from "a few pixels off the map" to
FLT_MAX, +-inf and NaN, and one placement of it over a small source grid.  TEST INFRASTRUCTURE ONLY.

A ladder value v is meant in the units of one target level l: the coordinate written is v * 2^l, which the level-l lookup
divides back to v exactly (every entry is representable in float32 at every scaling it is written at; asserted on
import).  At the other levels it is just another wild value.

Classes and what each is aimed at (R = lookup radius, n = the extent of the axis at the target level):
  edge    exact integers at the map edge and +-2^-10 beside them (dx == 0, the first / last tap that is still inside, the
          first window that is entirely outside, -0.0): what Gaussian-perturbed grids never produce
  i16     the int16 rails: kernels that pack window boxes as int16 pairs, saturating or truncating
  alias   65536 + 5.25 and friends: a truncating 16-bit pack maps them onto column 5; `twin` is the in-map 5.25
  m24     2^24 + 6 and friends: a 24-bit multiply maps the row onto row 6; twins 5, 6, 8
  i32     the int32 rails, where float -> int saturates and `floor - r + i` wraps
  nonfin  +-inf, NaN, +-subnormal
"""
import numpy as np

f32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.float32(1e-40))          # a float32 subnormal
E20 = float(np.float32(1e20))
EPS = 2.0 ** -10
ALL_LEVELS = (0, 1, 2, 3)


def _abs(v):
    return lambda n, R: v


_EDGE_INTS = [
    ("-(R+2)", lambda n, R: -(R + 2.0)), ("-(R+1)", lambda n, R: -(R + 1.0)), ("-R", lambda n, R: -float(R)),
    ("-1", _abs(-1.0)), ("-0.0", _abs(-0.0)), ("0", _abs(0.0)),
    ("n-1", lambda n, R: n - 1.0), ("n", lambda n, R: float(n)), ("n+R", lambda n, R: float(n + R)),
    ("n+R+1", lambda n, R: n + R + 1.0),
]


def _beside(fn, d):
    return lambda n, R: fn(n, R) + d


# (class, label, value(n, R), levels the entry may be written at[, group]); the entries of a group (aliases and their
# in-map twin) are written at the same level in the same pass, on neighbouring slots
LADDER = []
for _label, _fn in _EDGE_INTS:
    LADDER.append(("edge", _label, _fn, ALL_LEVELS))
    if _label != "-0.0":                 # -0.0 +- 2^-10 are the neighbours of 0 again
        LADDER.append(("edge", _label + "+2^-10", _beside(_fn, EPS), ALL_LEVELS))
        LADDER.append(("edge", _label + "-2^-10", _beside(_fn, -EPS), ALL_LEVELS))
LADDER += [
    ("i16", "32760", _abs(32760.0), ALL_LEVELS), ("i16", "32767", _abs(32767.0), ALL_LEVELS),
    ("i16", "32767.5", _abs(32767.5), ALL_LEVELS), ("i16", "32768", _abs(32768.0), ALL_LEVELS),
    ("i16", "32768+R+1", lambda n, R: 32768.0 + R + 1, ALL_LEVELS), ("i16", "-32768", _abs(-32768.0), ALL_LEVELS),
    ("i16", "-32769-R", lambda n, R: -32769.0 - R, ALL_LEVELS),
    ("alias", "65536+5.25", _abs(65536 + 5.25), ALL_LEVELS, "a"), ("twin", "5.25", _abs(5.25), ALL_LEVELS, "a"),
    ("alias", "-65536+5.25", _abs(-65536 + 5.25), ALL_LEVELS, "a"),
    ("alias", "131072+5.25", _abs(131072 + 5.25), ALL_LEVELS, "b"), ("twin", "5.25", _abs(5.25), ALL_LEVELS, "b"),
    ("m24", "2^23+5", _abs(2.0 ** 23 + 5), ALL_LEVELS, "c"), ("twin", "5", _abs(5.0), ALL_LEVELS, "c"),
    ("m24", "2^24+6", _abs(2.0 ** 24 + 6), ALL_LEVELS, "d"), ("twin", "6", _abs(6.0), ALL_LEVELS, "d"),
    ("m24", "-2^24+6", _abs(-2.0 ** 24 + 6), ALL_LEVELS, "d"),
    ("m24", "2^25+8", _abs(2.0 ** 25 + 8), ALL_LEVELS, "e"), ("twin", "8", _abs(8.0), ALL_LEVELS, "e"),
    ("i32", "2^30", _abs(2.0 ** 30), ALL_LEVELS), ("i32", "2^31-128", _abs(2.0 ** 31 - 128), ALL_LEVELS),
    ("i32", "2^31", _abs(2.0 ** 31), ALL_LEVELS), ("i32", "-2^31", _abs(-2.0 ** 31), ALL_LEVELS),
    ("i32", "-2^31-256", _abs(-2.0 ** 31 - 256), ALL_LEVELS), ("i32", "3e9", _abs(3e9), ALL_LEVELS),
    ("i32", "-3e9", _abs(-3e9), ALL_LEVELS), ("i32", "2^32+1024", _abs(2.0 ** 32 + 1024), ALL_LEVELS),
    ("i32", "1e20", _abs(E20), ALL_LEVELS), ("i32", "-1e20", _abs(-E20), ALL_LEVELS),
    # FLT_MAX * 2 is not a float32: it is written at level 0 alone
    ("i32", "FLT_MAX", _abs(FLT_MAX), (0,)), ("i32", "-FLT_MAX", _abs(-FLT_MAX), (0,)),
    ("nonfin", "+inf", _abs(float("inf")), ALL_LEVELS), ("nonfin", "-inf", _abs(float("-inf")), ALL_LEVELS),
    ("nonfin", "nan", _abs(float("nan")), ALL_LEVELS), ("nonfin", "1e-40", _abs(TINY), ALL_LEVELS),
    ("nonfin", "-1e-40", _abs(-TINY), ALL_LEVELS),
]
assert len(LADDER) == 64                 # edge 1 (192 pixels) carries every entry on x alone, on y alone and on both
PHASE, _first = [], {}
for _k, _e in enumerate(LADDER):
    PHASE.append(_first.setdefault(_e[4], _k) if len(_e) > 4 else _k)
CLASSES = ("edge", "i16", "alias", "twin", "m24", "i32", "nonfin")
AXES = ("x", "y", "both")

# every extent and radius the tests use: 24x32 slices and 8x24 maps, halved three times; radius 1..4 (4: gaussian mask)
EXTENTS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 30, 32)
RADII = (1, 2, 3, 4)


def value(k, n, R):
    """Ladder entry k in level units, for an axis of extent n and radius R."""
    return float(LADDER[k][2](n, R))


def written(k, n, R, level):
    """The float32 coordinate that carries entry k to `level`."""
    return f32(value(k, n, R) * 2.0 ** level)


def _check_representable():
    for k, (_, label, _, levels) in enumerate(e[:4] for e in LADDER):
        for n in EXTENTS:
            for R in RADII:
                v = value(k, n, R)
                for l in levels:
                    w = written(k, n, R, l)
                    if np.isnan(v):
                        assert np.isnan(w)
                        continue
                    assert float(w) == v * 2.0 ** l, (label, n, R, l)              # representable at this scaling
                    assert float(w / f32(2.0 ** l)) == v, (label, n, R, l)         # and the level divides it back
                    assert np.signbit(w) == np.signbit(v), (label, n, R, l)


_check_representable()


def slots(H1, W1):
    """(edge, flattened pixel) of every pixel that receives a ladder entry: every 5th pixel of edge 0 (wild and ordinary
    pixels share waves, 16-lane rows and tiles), every pixel of edge 1 (whole tiles with an empty window).  Edge 2 stays
    ordinary."""
    P = H1 * W1
    return [(0, p) for p in range(0, P, 5)] + [(1, p) for p in range(P)]


def schedule(H1, W1):
    """For every slot: (edge, pixel, ladder index, axis mode, level).  Edge 1 walks the table in order, one pass per axis
    mode (neighbouring pixels carry neighbouring entries: an alias next to its twin); edge 0 strides through it so that its
    few slots reach every class.  Each pass moves every entry on to its next level."""
    n = len(LADDER)
    out = []
    for k, (e, p) in enumerate(slots(H1, W1)):
        if e == 0:
            idx, pas = (11 * k) % n, k
        else:
            k -= len(range(0, H1 * W1, 5))
            idx, pas = k % n, k // n
        levels = LADDER[idx][3]
        out.append((e, p, idx, AXES[pas % 3], levels[(PHASE[idx] + pas) % len(levels)]))
    return out


def apply_ladder(coords_xy, extents, R):
    """coords_xy (3, H1, W1, 2) ordinary float32 coordinates in level-0 units, x first; extents[l] = (H2, W2) of target
    level l; a single extent = an operator without levels (every entry is written at level 0).  Returns the copy that
    carries the ladder."""
    E, H1, W1, _ = coords_xy.shape
    assert E == 3 and coords_xy.dtype == np.float32
    c = coords_xy.copy()
    for e, p, idx, axis, lv in schedule(H1, W1):
        lv = lv if len(extents) > 1 else 0
        h2, w2 = extents[lv]
        if axis in ("x", "both"):
            c[e, p // W1, p % W1, 0] = written(idx, w2, R, lv)
        if axis in ("y", "both"):
            c[e, p // W1, p % W1, 1] = written(idx, h2, R, lv)
    return c


# wild OFFSETS on single taps of otherwise ordinary pixels of edge 0 (none of them a multiple of 5): a pixel's window box
# is a reduction over its taps, so one wild tap must send the pixel to the per-tap path without losing the other taps.
# (pixel, tap (i, j) counted from the end when negative or None = the centre tap, which the kernels zero, component or
# None = both, value)
WILD_OFFSETS = ((106, (0, 1), 0, float("nan")), (107, (-1, 0), None, 1e6), (108, (1, -1), 1, -40000.0), (109, None, None, float("nan")))


def apply_wild_offsets(offset, R, shift=0):
    """offset (>=1, H1, W1, rd, rd, 2): write WILD_OFFSETS into row 0, at pixels moved on by `shift` (so that two levels
    carry them on different pixels).  In place; returns the pixels touched."""
    W1 = offset.shape[2]
    rd = 2 * R + 1
    touched = []
    for p, tap, comp, v in WILD_OFFSETS:
        p += shift
        assert p % 5 != 0
        i, j = (R, R) if tap is None else (tap[0] % rd, tap[1] % rd)
        assert tap is None or (i, j) != (R, R)
        sl = slice(None) if comp is None else comp
        offset[0, p // W1, p % W1, i, j, sl] = v
        touched.append(p)
    return touched


def grid_xy(rng, E, H1, W1, sigma=3.0):
    """grid + N(0, sigma^2), (E, H1, W1, 2), x first."""
    ys, xs = np.meshgrid(np.arange(H1, dtype=np.float32), np.arange(W1, dtype=np.float32), indexing="ij")
    g = np.stack([xs, ys], -1)[None].repeat(E, 0)
    return (g + rng.standard_normal((E, H1, W1, 2)).astype(np.float32) * sigma).astype(np.float32)


H1, W1 = 8, 24                           # source grid: 1.5 tiles of the metric kernel, 2 x 3 of the cooperative kernel
VOL_EXTENTS = [(24 >> l, 32 >> l) for l in range(4)]
MAP_EXTENTS = [(8 >> l, 24 >> l) for l in range(4)]


def volume_case(R=3, seed=9100):
    """Three edges over the 8 x 24 source grid, target slices 24 x 32 over four levels.  Returns dict(volumes, coords
    (3,2,8,24) with the ladder, plain (the same with edges 0 and 1 ordinary), offsets (four dense levels, levels 0-1 with
    the wild taps))."""
    rng = np.random.default_rng(seed + R)
    rd = 2 * R + 1
    vols = [rng.standard_normal((3, H1, W1, h, w)).astype(np.float32) for h, w in VOL_EXTENTS]
    xy = grid_xy(rng, 3, H1, W1)
    offs = [(4 * np.tanh(rng.standard_normal((3, H1, W1, rd, rd, 2)))).astype(np.float32) for _ in range(4)]
    offs[1] = ((offs[1] + offs[0]) / 2).astype(np.float32)
    apply_wild_offsets(offs[0], R)
    apply_wild_offsets(offs[1], R, shift=5)
    wild = apply_ladder(xy, VOL_EXTENTS, R)
    tr = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))
    return dict(volumes=vols, coords=tr(wild), plain=tr(xy), offsets=offs)


def map_case(C, R=3, seed=9200):
    """Low-memory path: three edges, feature maps 8 x 24 halved per level.  coords (3,1,8,24,2)."""
    rng = np.random.default_rng(seed + C + R)
    rd = 2 * R + 1
    f1 = (rng.standard_normal((3, H1, W1, C)) * 0.125).astype(np.float32)
    f2s = [(rng.standard_normal((3, h, w, C)) * 0.125).astype(np.float32) for h, w in MAP_EXTENTS]
    xy = grid_xy(rng, 3, H1, W1)
    offs = [(4 * np.tanh(rng.standard_normal((3, H1, W1, rd, rd, 2)))).astype(np.float32) for _ in range(2)]
    offs[1] = ((offs[1] + offs[0]) / 2).astype(np.float32)
    apply_wild_offsets(offs[0], R)
    apply_wild_offsets(offs[1], R, shift=5)
    wild = apply_ladder(xy, MAP_EXTENTS, R)
    return dict(fmap1=f1, fmap2s=f2s, coords=wild[:, None].copy(), plain=xy[:, None].copy(), offsets=offs)


def gauss_case(W2, R=4, seed=9300):
    """gaussianMask: volume (3,8,24,24,W2), the means carry the ladder (one level), covs ~ U(0.05, 5.05)."""
    rng = np.random.default_rng(seed + W2)
    vol = rng.standard_normal((3, H1, W1, 24, W2)).astype(np.float32)
    xy = grid_xy(rng, 3, H1, W1, 2.0)
    covs = rng.uniform(0.05, 5.05, (3, H1, W1, 2)).astype(np.float32)
    grad = rng.standard_normal(vol.shape).astype(np.float32)
    return dict(volume=vol, means=apply_ladder(xy, [(24, W2)], R), plain=xy, covs=covs, grad=grad, radius=R)


def build_case(C=32, H=8, Wd=32, R=4, seed=9400):
    """The fused pyramid builder: feature maps (3, C, H, Wd) whose all-pairs volume is (3, H, Wd, H, Wd); the means carry the
    ladder over that H x Wd grid."""
    rng = np.random.default_rng(seed + C)
    f1 = (rng.standard_normal((3, C, H, Wd)) * 0.5).astype(np.float32)
    f2 = (rng.standard_normal((3, C, H, Wd)) * 0.5).astype(np.float32)
    xy = grid_xy(rng, 3, H, Wd, 1.5)
    covs = rng.uniform(0.05, 5.05, (3, H, Wd, 2)).astype(np.float32)
    return dict(fmap1=f1, fmap2=f2, means=apply_ladder(xy, [(H, Wd)], R), covs=covs, radius=R)


def tame(c, limit=2.0 ** 30, fill=1.0e4):
    """The coordinates restricted to what C defines: finite and |c| <= 2^30; the others become `fill` (off every map)."""
    c = c.copy()
    c[~(np.abs(c) <= limit)] = fill
    return c

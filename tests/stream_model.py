"""A float64 model of the PRODUCTION photon streams in a horizontally uniform medium, written from the convention as
csrc/philox.hpp (PhiloxStreamT), csrc/kernels.hpp (photon_kernel: parts A to C of the event phase, make_ray) and csrc/tracer.hpp
(scattering_cosine<false>, next_direct, lookup_phase_fast) state it.  Plain numpy; of the product it imports nothing, and of the
tests only tests/philox_ref.py (the scalar Philox that `philox` below is held against).

What the model follows (the line it restates in brackets):
  * key (seed0, seed1), counter (photon_lo, photon_hi, block, 0); block 0 of a photon gives start x, start y and the first optical
    depth, block k its k-th event; next() -- the component choice -- refills from the SAME block counter, four deviates a block
    [PhiloxStreamT::make_block, begin_event, next];
  * deviate = float32(float64(u) / (2^32 - 1)) [u32_to_unit_float];
  * roles: first() scattering angle | start x | cosine of a reflection; second() azimuth | start y; path() optical depth; spare()
    roulette [philox.hpp, the comment above PhiloxStreamT];
  * the scattering cosine in float32, operation by operation, with quirk Q1 (`left` is not rescaled by n) [scattering_cosine<false>];
    1 - cos^2 in float32 as well (near-forward scattering is badly conditioned there: the model must not be better than the kernel);
  * the new direction: next_direct's formula in float64, azimuth 2 pi second() [next_direct, disc_point];
  * surface: mu = sqrt(first()), azimuth second(), weight times albedo; a black surface ends a photon of a flux kernel without a
    block being drawn, a radiance kernel draws the block and its two deviates first [part A `atBlack`, part C];
  * components: 1 + number of the cell's first ncomp - 1 cumulative extinction fractions at or below the deviate [part C, MULTI];
  * absorption w (1 - omega) into the cell, then w omega; roulette below 0.5: spare() >= w ends the photon, else w = 1 [part C];
  * radiance, plain local estimate: w P(theta) / (4 pi |mu_d|) exp(-tau) per event and direction, the surface's w / pi exp(-tau), into
    the column in which the RAY leaves the domain [service phase: `(sr.iy - 1) * nx + (sr.ix - 1)`]; hybrid tables for orders up
    to numOrdersOrig; the contribution limit [make_ray, service phase];
  * the local estimate's own roulette (rr_intensity, Iwabuchi's; zeta_min): a ray's block is philox(photon_lo, photon_hi, the photon's
    block counter as the event leaves it, direction + 1; the photon's key) -- word 0 its free path tauFree = -log(max(tiny, u0)), word 1
    its roulette deviate r2, two deviates a ray whether it is traced or not [philox.hpp, the comment above PhiloxStreamT; make_ray].
    pi norm <= zetaMin, a SMALL contribution: won = r2 zetaMin <= pi norm is decided before any trace; a lost ray adds nothing and counts
    as skipped (I3RC_CNT_RAYS_SKIPPED); a won one adds w zetaMin / pi if the top lies within tauFree, else 0.  A LARGE one: tauMax =
    -log(zetaMin / (pi norm)); the top within tauMax: the plain estimate; a first leg that leaves through the bottom: 0; else a second
    leg from where the first one arrives, target tauFree: w zetaMin / pi if it leaves through the top, else 0.  A downward direction
    never counts: its entries are exactly 0 (Result.exact_zero).  The contribution limit applies to whichever value results [make_ray,
    service phase];
  * counters, and the deviates consumed one by one (I3RC_CNT_RNG_DRAWS); I3RC_CNT_TRACER_CALLS: one per trace of a photon, per traced
    ray and per second leg;
  * the one diagnostic tally of a flux launch (Problem.extra; ExtraTally in tally_block.hpp), each from what the general flux kernel
    photon_kernel<Philox{Level,Track,Path,Bin}Stream, false, true, GRID> states:
      the path L of a photon: 0 at its start -- the start height zstart, not the top -- [part C, ST_NEW: `pathLen = 0.0`], + the
        geometric length |s| of every traced segment [photon_step: `pathLen += (double)len` per voxel step that is no tracer error;
        the event phase: `pathLen += (double)part`, finish_arrival<true>], carried through a surface reflection (nothing resets it there);
      "paths"  pathUp1 | pathUp2 | pathDown1 | pathDown2 [ny, nx]: w L and w L^2 where and in the column where fluxUp / fluxDown are
        tallied [path_add beside tally.boundary in part A, beside tally.down in part C], a surface arrival with the weight BEFORE
        the reflection [path_add stands before `w = w * Pe.albedo`];
      "bins"   binUp | binPathUp | binDown | binPathDown [nBins + 1], overflow last: w and w L at the same places into the bin b of
        float32(L) with edges[b] <= x < edges[b + 1] [bin_add: `(float)length`; path_bin];
      "levels" levelFluxUp | levelFluxDown [nz + 1, ny, nx]: a new photon adds 1 to levelFluxDown at the level behind its start layer
        in its start column [part C, ST_NEW: `down ? r.iz : r.iz - 1`]; a segment from layer a to layer b (1-based; nz + 1 out through
        the top, 0 onto the surface) adds w to levelFluxUp[a .. b - 1] going up, to levelFluxDown[b .. a - 1] going down [part A:
        tally_level_crossings with izFrom -- set where the trace starts -- and izTo]; the level the segment ENDS on (top, surface) takes
        the arrival's own column, every other level the column of the point where the straight segment meets ze[k], wrapped
        periodically [tally_level_crossings: extrapolated back from the arrival, find_xy]; a reflected photon that goes on adds its
        weight AFTER the reflection to levelFluxUp[0] in the column where it was reflected [part C: `add_global(... + c2, w)`];
      "tracks" [nz, ny, nx]: every segment cut by the planes of the grid (float64, periodic in x and y); each piece adds w l to the cell
        it lies in, w the weight along the segment, before the event at its end [photon_step: track_add of the cell BEFORE the step;
        the event phase: the arrival's part in the cell the photon stands in]; `trackLayers` [nz]: the same added over a layer's columns.
The optical path is analytic: with C(z) the extinction integrated from the bottom, a path of optical depth tau along direction
cosine dz ends where C changes by tau |dz|.  The tracer itself is pinned bit for bit elsewhere (tests/test_gpu_parity.py).

Out of scope (the replay pin and the oracle tests cover them): max cross-section, gridded surfaces, explicit photon sources,
horizontally varying fields, zetaMin = 0, a reflection's retry (a deviate of exactly 0: asserted not to occur); of the diagnostic
tallies the fused and moments entry points (they refuse or wrap the kinds: tests/test_gpu_diagnostic_moments.py) and the workgroup's
LDS sums as such (the same additions in another order: the kinds' own suites).

MARGINS AND BOUNDS.  Every discrete decision records its margin and the model's own bound on the float32 error of the compared
quantity; a photon is FRAGILE when some margin is below 4 bounds.  The decisions: top / bottom / which layer (one comparison of
optical depths), the component compare (both sides are float32 values the kernel holds too: bound 0), the roulette compares
(w < 0.5, spare >= w), the column of an event, an exit or a ray's exit, the sign of the direction's z-cosine in next_direct (its
frame changes hands there) and the contribution limit; with a diagnostic tally also the START COLUMN of a new photon (levels; bound: the
start position's e_h = 2 eps |x|max, the product and the sum of x0 + u (xMax - x0)), the LEVEL COLUMN of every crossing that is not the
segment's end (levels; bound below) and the BIN of float32(L) (bins; margin: the distance of L to the two edges that bracket it, bound
e_L + eps L, the conversion's rounding); with the local estimate's roulette also pi norm against zetaMin (bound: pi e_norm
+ 3 eps of the product), r2 zetaMin against pi norm (+ 1 eps), the optical depth to the top against tauFree (e_tau + 2 ulp for fast_log)
and against tauMax (e_tau + 2 ulp + 1 ulp for fast_div + 3 eps + e_norm / norm), the second leg's remaining depth against tauFree (all
of these, + the arrival point's rounding) -- each only where its outcome reaches a tally or a counter, and a ray's column only where
the ray counts.  The capped value w zetaMin (1 / pi) is formed with the float32 constant: the weight's bound + 3 eps.  The table
intervals are no such decisions here: the inverse table's k comes from a float32 product the model forms bit for bit, and the forward table's interpolation is continuous across k -- a neighbouring
interval is within what P at theta +- e_theta already allows.  The bound is first order and summed along
the photon's events from what the code states: hardware sin / cos 1e-7 absolute, fast_log 2 ulp, v_rcp / v_sqrt / v_exp 1 ulp, one
rounding (2^-24 relative) per float32 operation otherwise, one ulp for the scattering cosine wherever refined_rcp(n) one ulp off the
correctly rounded 1 / n would give another one (evaluated per event):
  height          kept as e_C, the error of C(z): e_C + |dz| (2 ulp tau + 3 eps steps tau_path) + (side faces + 1) eps (|z|max + 2 dz) ext_max
                  + tau_path e_dir, which is what the comparison with the layers' faces, the top and the bottom sees (a coordinate is
                  exact on a face it has just reached: z is rounded only where a side face is crossed); + 4 eps |z|max ext at the event
  x, y            e_xy + s e_dir + |d| e_s + steps eps (|x|max + 2 dx),  e_s = (e_C' / ext' + e_C / ext) / |dz| + s e_dir / |dz|
  direction       gain e_dir + [ulp / sin(theta) where the cosine is not certain to the bit] + 1e-7 sqrt2 sin(theta) + 3 ulp sin(theta) + 10 eps,  gain = the rotation's own
                  Lipschitz constant at that event: the largest singular value of its finite-difference Jacobian on the tangent plane
  weight          one eps per factor
  radiance        the weight's, P at theta +- e_theta (evaluated, not linearised), exp at tau +- e_tau, 1 ulp each for v_rcp / v_exp
  path L          e_L = the sum over the segments of e_s + steps eps |s|: the along-path error above, one float32 rounding per voxel-step
                  piece (`step`, a quotient) and for the arrival piece (finish_arrival's exact_div); the float64 additions add nothing
  paths           per deposit w (e_w L + e_L) for w L, w (e_w L^2 + 2 L e_L) for w L^2
  bins            w e_w for the weights, the bound of w L for binPath
  levels          w e_w per deposit; the level column's bound: the arrival's e_xy + back e_dir (back: the path from the crossing to the
                  arrival) + eps (3 h + 4 (|x|max + h) + |x|max), h = |d_xy| back, for tally_level_crossings' float32 operations: back =
                  (z - zE[k]) / dz (a difference, a quotient) and dx * back (a product): 3 eps h; x - dx * back, the wrap's difference
                  and quotient inside floorf and its product by the width: eps (|x|max + h) each; the last difference: eps |x|max; the
                  clamp rounds nothing
  tracks          per piece w (e_w l + e_l), e_l = eps l (the piece's quotient) + l e_dir / |dz| + (side faces crossed before it in the
                  segment) eps (|z|max + 2 dz) / |dz| (z is rounded only where a side face is crossed) + for the first piece the start's
                  along-path error e_C / ext / |dz|, for the last one the arrival's e_C' / ext' / |dz| (the two terms of e_s); per side
                  face crossed, in BOTH adjoining cells, the transfer w min(e_xy / |d_n|, the two adjoining pieces' lengths), d_n the
                  cosine normal to the face: the position's error moves length continuously from a cell to its neighbour -- no discrete
                  decision; the per-layer sums carry no transfer terms
(steps: voxel faces crossed + 1).  No constant in it is fitted to what a kernel gives.

A FRAGILE PHOTON AND THE DIAGNOSTIC TALLIES.  The caps (a weight is at most 1 per tally) do not extend to a path, which has no upper
limit: the diagnostic fields are compared only over photons that are not fragile -- clean_runs gives all maximal runs of them, run(ids=...)
the model over exactly those photons -- and compare() refuses anything else.

Measured with `python -m tests.stream_model` (fragile photons / photons, per shared case; the cap tests/test_stream_model_cpu.py
asserts is 0.5 %): see FRAGILE_SHARES at the end of this module, and DIAGNOSTIC_SHARES for the diagnostic cases and kinds."""
import ctypes
import ctypes.util
from dataclasses import dataclass, field

import numpy as np

from tests.philox_ref import M0, M1, W0, W1   # (the multipliers and Weyl constants: one statement of them)

f32, f64 = np.float32, np.float64
EPS, ULP, SINCOS = 2.0 ** -24, 2.0 ** -23, 1e-7
TINY = float(np.finfo(np.float32).tiny)
PI32 = f32(3.14159265358979312)
SAFETY = 4.0
_M0, _M1, _W0, _W1, _MASK = (np.uint64(v) for v in (M0, M1, W0, W1, 0xFFFFFFFF))
_S32 = np.uint64(32)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("cosf", "sinf", "sqrtf"):
    getattr(_libm, _n).argtypes, getattr(_libm, _n).restype = [ctypes.c_float], ctypes.c_float


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (uint64 holding 32-bit words); scalars broadcast."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, np.uint64) & _MASK for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> _S32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def unit(u):
    """deviate of a 32-bit word, as a float64 holding the float32 value"""
    return (np.asarray(u, np.uint64).astype(f64) / 4294967295.0).astype(f32).astype(f64)


def direction(mu, phi_deg):
    """makeDirectionCosines as the host evaluates it (float32, libm)"""
    mu = f32(mu)
    phi = f32(f32(f32(phi_deg) * f32(np.arccos(f32(-1.0)))) / f32(180.0))
    st = f32(_libm.sqrtf(f32(f32(1.0) - f32(mu * mu))))
    return np.array([f32(st * f32(_libm.cosf(phi))), f32(st * f32(_libm.sinf(phi))), mu], f32)


EXTRAS = (None, "levels", "tracks", "paths", "bins")
# the fields of each kind's block, in the block's order (tally_block.hpp: ExtraTally, tally_layout, path_bin_field); `trackLayers` is
# no field of the device's: the track sums added over the columns of a layer, which the caller forms from the block
EXTRA_FIELDS = {None: (), "levels": ("levelFluxUp", "levelFluxDown"), "tracks": ("tracks",),
                "paths": ("pathUp1", "pathUp2", "pathDown1", "pathDown2"), "bins": ("binUp", "binPathUp", "binDown", "binPathDown")}
DERIVED_FIELDS = ("trackLayers",)


@dataclass
class Problem:
    xe: np.ndarray
    ye: np.ndarray
    ze: np.ndarray
    ext: np.ndarray                 # [ncomp, nz] float32
    ssa: np.ndarray                 # [ncomp, nz]
    pfi: np.ndarray                 # [ncomp, nz] table entry, 1-based (0 where there is no extinction)
    inv: list                       # per component [nEntries, nInv] scattering angles, as handed to the device
    mu0: float = 1.0
    azimuth: float = 0.0
    albedo: float = 0.0
    roulette: bool = True
    dirs: np.ndarray = None         # [nDir, 3] float32 direction cosines, as handed to the device
    fwd: list = None                # per component [nEntries, nFwd]: the table in use (the hybrid one where that is on)
    fwd_orig: list = None           # ... and the original phase functions (orders <= orders_orig with hybrid on)
    hybrid: bool = False
    orders_orig: int = 0
    max_contrib: float = None       # the contribution limit; None: off
    rr_intensity: bool = False      # the local estimate's own roulette (useRussianRouletteForIntensity)
    zeta_min: float = 0.3           # ... and its bound (the library's default)
    extra: str = None               # the one diagnostic tally of the launch (EXTRAS; ExtraTally in tally_block.hpp), flux launches only
    bin_edges: np.ndarray = None    # extra == "bins": the nBins + 1 float32 edges as handed to the device (edges[0] == 0, ascending)

    def __post_init__(self):
        self.xe, self.ye, self.ze = (np.asarray(a, f32) for a in (self.xe, self.ye, self.ze))
        self.ext, self.ssa = np.atleast_2d(np.asarray(self.ext, f32)), np.atleast_2d(np.asarray(self.ssa, f32))
        self.pfi = np.atleast_2d(np.asarray(self.pfi, np.int64))
        self.inv = [np.atleast_2d(np.asarray(t, f32)) for t in self.inv]
        assert self.extra in EXTRAS, self.extra
        assert self.extra is None or self.dirs is None, "the diagnostic tallies refuse radiance directions"
        if self.extra == "bins":
            self.bin_edges = np.asarray(self.bin_edges, f32)
            assert self.bin_edges[0] == 0 and np.all(np.diff(self.bin_edges) > 0)
        if self.dirs is not None:
            self.dirs = np.asarray(self.dirs, f32).reshape(-1, 3)
            self.fwd = [np.atleast_2d(np.asarray(t, f32)) for t in self.fwd]
            self.fwd_orig = self.fwd if self.fwd_orig is None else [np.atleast_2d(np.asarray(t, f32)) for t in self.fwd_orig]

    @property
    def ndir(self):
        return 0 if self.dirs is None else len(self.dirs)


@dataclass
class Result:
    n: int
    tallies: dict
    bounds: dict
    counters: dict
    per_photon: dict                # fate (0 top, 1 surface, 2 roulette / absorbed), order, weight, fragile, counts, deposits
    caps: dict = field(default_factory=dict)
    branches: dict = field(default_factory=dict)   # rays of the local estimate's roulette by what became of them (BRANCHES)
    extras: dict = field(default_factory=dict)     # the diagnostic kinds' own records: per-photon sums, the pieces a cell received
    exact_zero: dict = field(default_factory=dict)  # per tally: entries nothing can reach, whatever a fragile photon does (a downward direction's, with the roulette)

    @property
    def fragile_share(self):
        return float(self.per_photon["fragile"].mean())


VARIANTS = ("swap first second", "azimuth from first", "table interval k + 1")
# ... and of the local estimate's roulette (rr_intensity): each one a mistake the kernels could make in make_ray or the service phase
RAY_VARIANTS = ("ray block ignores the direction", "ray counter word d", "r2 from word 0", "ray key without the batch", "ray block without the high word",
                "second leg from the event", "downward direction counts")
# what a ray of the roulette can do (Result.branches counts the rays of each)
BRANCHES = ("small lost", "small won counted", "small won ended inside", "large first leg", "large through the bottom",
            "second leg counted", "second leg ended inside", "surface small", "surface large", "capped above the limit")


# ... and of the diagnostic tallies: each one another convention for the path register, the level ranges or the pieces of a track
EXTRA_VARIANTS = {"paths": ("path restarts at a reflection", "surface tally with the weight after the reflection", "last segment left out of L"),
                  "bins": ("path restarts at a reflection", "surface tally with the weight after the reflection", "last segment left out of L",
                           "bin of L before the last segment"),
                  "levels": ("crossing counted in the arrival column", "new photon not counted", "downward range shifted by one level",
                             "reflected photon not counted"),
                  "tracks": ("weight after the scattering", "piece credited to the cell after the step", "arrival piece left out")}


def run(P, seed, first_photon, n, variant=None, drop_high_word=False, batch=0, ids=None):
    """n photons first_photon .. first_photon + n - 1 of the key (seed[0], seed[1] + batch): batch `batch` of a fused launch whose
    first batch has the key `seed`.  ids: the photon numbers themselves instead (any set of them: photons do not know of each other)"""
    assert variant is None or variant in VARIANTS + RAY_VARIANTS + EXTRA_VARIANTS.get(P.extra, ()), variant
    if ids is not None:
        n = len(ids)
    nx, ny, nz, ncomp = len(P.xe) - 1, len(P.ye) - 1, len(P.ze) - 1, P.ext.shape[0]
    xe, ye, ze = P.xe.astype(f64), P.ye.astype(f64), P.ze.astype(f64)
    x0, y0, Lx, Ly = xe[0], ye[0], xe[-1] - xe[0], ye[-1] - ye[0]
    # the host's sums (float32, component after component) and cumulative fractions
    cum32 = np.cumsum(P.ext, axis=0, dtype=f32).astype(f32)
    tot32 = cum32[-1]
    frac = np.where(tot32 > TINY, cum32 / np.where(tot32 > TINY, tot32, f32(1)), cum32).astype(f32).astype(f64)
    ext = tot32.astype(f64)
    cumz = np.concatenate([[0.0], np.cumsum(ext * np.diff(ze))])
    extmax = float(ext.max())
    zs, xs = float(np.abs(ze).max()), float(max(np.abs(xe).max(), np.abs(ye).max()))
    dzmax, dxmax = float(np.diff(ze).max()), float(max(np.diff(xe).max(), np.diff(ye).max()))
    cosT = [np.cos(t.astype(f64)).astype(f32) for t in P.inv]
    nd = P.ndir
    black = not (f32(P.albedo) > TINY) and nd == 0
    alb = float(f32(P.albedo))
    k0, k1 = np.uint64(seed[0] & 0xFFFFFFFF), np.uint64((seed[1] + batch) & 0xFFFFFFFF)
    k1_ray = np.uint64(seed[1] & 0xFFFFFFFF) if variant == "ray key without the batch" else k1   # (a ray's key is its photon's)
    zeta = float(f32(P.zeta_min))
    inv_pi32 = float(f32(1.0) / PI32)   # the float32 constant 1 / pi of the capped value
    branches = {k: 0 for k in BRANCHES}
    pid = np.uint64(first_photon) + np.arange(n, dtype=np.uint64) if ids is None else np.asarray(ids, np.uint64)
    lo, hi = pid & _MASK, (np.zeros(n, np.uint64) if drop_high_word else pid >> _S32)

    T = dict(fluxUp=np.zeros((ny, nx)), fluxDown=np.zeros((ny, nx)), volumeAbsorption=np.zeros((nz, ny, nx)),
             intensity=np.zeros((ncomp + 1, max(nd, 1), ny, nx)), intensityExcess=np.zeros((ncomp + 1, max(nd, 1))))
    extra = P.extra
    path_kind = extra in ("paths", "bins")
    edges = P.bin_edges.astype(f64) if extra == "bins" else None
    nbins = len(edges) - 1 if extra == "bins" else 0
    shapes = {"levels": (nz + 1, ny, nx), "tracks": (nz, ny, nx), "paths": (ny, nx), "bins": (nbins + 1,)}
    for k in EXTRA_FIELDS[extra]:
        T[k] = np.zeros(shapes[extra])
    if extra == "tracks":
        T["trackLayers"] = np.zeros(nz)
    Bd = {k: np.zeros_like(v) for k, v in T.items()}
    # the kinds' own records.  perPhoton: each field's sum over the photon's deposits (levels: per level; `absLayer` what the photon
    # leaves in each layer as absorption; `wS` the sum of w |s| over its segments); trackPieces: the pieces a cell received
    X = dict(perPhoton={k: np.zeros((n,) + ((nz + 1,) if extra == "levels" else ())) for k in EXTRA_FIELDS[extra]})
    if extra == "levels":
        X["perPhoton"]["absLayer"] = np.zeros((n, nz))
    if extra == "tracks":
        X["perPhoton"]["wS"], X["trackPieces"] = np.zeros(n), np.zeros((nz, ny, nx), np.int64)
    if path_kind:
        X["deposits"] = []
    Lp, e_L = np.zeros(n), np.zeros(n)      # PATH: the photon's geometric path since its start [pathLen, kernels.hpp], and its error
    cnt = {k: np.zeros(n, np.int64) for k in ("scatterings", "surfaceHits", "exitsTop", "roulette", "rngDraws", "raysSkipped", "tracerCalls")}
    dep = {k: np.zeros(n) for k in ("fluxUp", "fluxDown", "volumeAbsorption", "intensity")}
    fragile, why = np.zeros(n, bool), {}
    fate, order, wfin = np.full(n, -1), np.zeros(n, np.int64), np.zeros(n)

    def decide(idx, margin, bound, kind):
        bad = margin < SAFETY * bound
        if bad.any():
            fragile[idx[bad]] = True
            why[kind] = why.get(kind, 0) + int(bad.sum())

    def roles(idx, blk):
        e = philox(lo[idx], hi[idx], blk, 0, k0, k1)
        u = [unit(w) for w in e]
        if variant == "swap first second":
            u[0], u[1] = u[1], u[0]
        return u

    def column(idx, xu, yu, ex_, who):
        """periodic wrap, column and the faces crossed on the way from the photon's current column"""
        kx, ky = np.floor((xu - x0) / Lx), np.floor((yu - y0) / Ly)
        xw, yw = xu - kx * Lx, yu - ky * Ly
        ci = np.clip(np.searchsorted(xe, xw, side="right") - 1, 0, nx - 1)
        cj = np.clip(np.searchsorted(ye, yw, side="right") - 1, 0, ny - 1)
        m = np.minimum(np.minimum(xw - xe[ci], xe[ci + 1] - xw), np.minimum(yw - ye[cj], ye[cj + 1] - yw))
        if who:
            decide(idx, m, ex_, who)
        crossed = np.abs(kx * nx + ci - cix[idx]) + np.abs(ky * ny + cj - ciy[idx])
        return xw, yw, ci, cj, crossed

    def rotate(s, cosS, sinT, turn):
        ang = 2.0 * np.pi * turn
        ax, ay = sinT * np.cos(ang), sinT * np.sin(ang)
        b = s[0] * ax - s[1] * ay
        dd = cosS - b / (1.0 + np.abs(s[2]))
        return np.array([s[0] * dd + ax, s[1] * dd - ay, s[2] * cosS - np.copysign(np.abs(b), s[2] * b)])

    def radiance(idx, comp, px, py, pz, din, wgt, e_c, e_h, e_dir, e_w, ordr):
        """the local estimate of the events `idx` (comp 0: the surface), every direction"""
        for d in range(nd):
            u = P.dirs[d].astype(f64)
            up = u[2] > 0
            zb = ze[-1] if up else ze[0]
            s = (zb - pz) / u[2]
            Cz = np.interp(pz, ze, cumz)
            tauB = np.abs((cumz[-1] if up else 0.0) - Cz) / abs(u[2])
            lay = np.clip(np.searchsorted(ze, pz, side="right") - 1, 0, nz - 1)
            ds = e_c / np.where(ext[lay] > 0, ext[lay], 1.0) / abs(u[2])
            exy = e_h + max(abs(u[0]), abs(u[1])) * ds
            crossed = column(idx, px + u[0] * s, py + u[1] * s, None, None)[4]
            steps = (nz - lay if up else lay + 1) + crossed + 1
            _, _, ci, cj, _ = column(idx, px + u[0] * s, py + u[1] * s, None, None)
            e_col = exy + steps * EPS * (xs + 2 * dxmax)
            e_tau = (e_c + extmax * (crossed + 1) * EPS * (zs + 2 * dzmax)) / abs(u[2]) + 3 * EPS * steps * tauB
            if comp is None:
                norm, e_norm = np.full(len(idx), 1.0 / np.pi), np.zeros(len(idx))
                cidx = np.zeros(len(idx), np.int64)
            else:
                cidx = comp
                proj = np.clip(din[0] * u[0] + din[1] * u[1] + din[2] * u[2], -1.0, 1.0)
                e_proj = e_dir + 4 * EPS
                theta = np.arccos(proj)
                e_th = np.minimum(e_proj / np.sqrt(np.maximum(1.0 - proj * proj, 1e-300)), np.sqrt(2 * e_proj)) + 4 * EPS * np.pi
                norm, e_norm = np.zeros(len(idx)), np.zeros(len(idx))
                for c in range(1, ncomp + 1):
                    for orig in (False, True):
                        sel = (comp == c) & ((P.hybrid & (ordr <= P.orders_orig)) == orig)
                        if not sel.any():
                            continue
                        tab = (P.fwd_orig if orig else P.fwd)[c - 1].astype(f64)
                        rows = tab[pfi_ev[sel] - 1]
                        th = theta[sel]
                        val, pos = _rowwise(rows, th)
                        vlo, _ = _rowwise(rows, np.clip(th - e_th[sel], 0.0, np.pi))
                        vhi, _ = _rowwise(rows, np.clip(th + e_th[sel], 0.0, np.pi))
                        norm[sel] = val / (4.0 * np.pi * abs(u[2]))
                        e_norm[sel] = (np.maximum(np.abs(vlo - val), np.abs(vhi - val)) + 4 * EPS * np.abs(val)) / (4.0 * np.pi * abs(u[2]))
            att = np.exp(-tauB)
            con = wgt * norm * att
            e_con = con * (e_w + 4 * EPS + 3 * ULP + 2 * EPS * tauB + np.expm1(e_tau)) + wgt * e_norm * att
            counted = np.ones(len(idx), bool)      # does the ray reach a tally at all?  (its column is a decision only then)
            capped = np.zeros(len(idx), bool)
            if not P.rr_intensity:
                cnt["tracerCalls"][idx] += 1
            else:
                # the ray's own block: same photon, the photon's block counter as the event leaves it (a component deviate that refilled
                # next() has moved it on: philox.hpp), the direction number + 1 in the fourth word; key as the photon's
                d4 = {"ray block ignores the direction": 1, "ray counter word d": d}.get(variant, d + 1)
                hi_ray = np.zeros(len(idx), np.uint64) if variant == "ray block without the high word" else hi[idx]
                q = philox(lo[idx], hi_ray, blk[idx] - 1, d4, k0, k1_ray)
                u0, r2 = unit(q[0]), unit(q[0] if variant == "r2 from word 0" else q[1])
                cnt["rngDraws"][idx] += 2
                tau_free = -np.log(np.maximum(TINY, u0))
                e_tf = 2 * ULP * tau_free
                reaches = up or variant == "downward direction counts"   # only an exit through the top counts
                pn = np.pi * norm
                e_pn = np.pi * e_norm + 3 * EPS * pn                   # (the product's rounding, pi's and -- the surface -- 1 / pi's)
                decide(idx, np.abs(pn - zeta), e_pn, "ray: small or large")
                small = pn <= zeta
                # small contribution: the roulette is decided before any trace; a lost ray is not traced
                decide(idx[small], np.abs(r2 * zeta - pn)[small], (e_pn + EPS * r2 * zeta)[small], "ray: won")
                won = small & (r2 * zeta <= pn)
                lost = small & ~won
                cnt["raysSkipped"][idx[lost]] += 1
                cnt["tracerCalls"][idx[~lost]] += 1
                if reaches:
                    decide(idx[won], np.abs(tauB - tau_free)[won], (e_tau + e_tf)[won], "ray: free path")
                won_top = won & (tauB <= tau_free) & reaches
                # large contribution: a first leg up to tauMax, a second one from where that arrives up to the free path
                large = ~small
                tau_max = -np.log(zeta / np.maximum(TINY, pn))
                e_tm = 2 * ULP * np.abs(tau_max) + ULP + 3 * EPS + e_norm / np.maximum(norm, TINY)
                decide(idx[large], np.abs(tauB - tau_max)[large], (e_tau + e_tm)[large], "ray: tauMax")
                first = large & (tauB <= tau_max)
                second = large & ~first
                cnt["tracerCalls"][idx[second]] += 1
                rem = tauB if variant == "second leg from the event" else tauB - tau_max
                e_rem = e_tau + e_tm + e_tf + 4 * EPS * zs * extmax / abs(u[2])   # (+ the arrival point's own rounding)
                if reaches:
                    decide(idx[second], np.abs(rem - tau_free)[second], e_rem[second], "ray: second leg")
                second_top = second & (rem <= tau_free) & reaches
                direct = first & reaches
                capped = won_top | second_top
                counted = direct | capped
                cap_val = wgt * zeta * inv_pi32
                con = np.where(direct, con, np.where(capped, cap_val, 0.0))
                e_con = np.where(direct, e_con, np.where(capped, cap_val * (e_w + 3 * EPS), 0.0))
                for k, m in (("small lost", lost), ("small won counted", won_top), ("small won ended inside", won & ~won_top & up),
                             ("large first leg", direct), ("large through the bottom", first & (not up)), ("second leg counted", second_top),
                             ("second leg ended inside", second & ~second_top & up), ("surface small", small & (comp is None)),
                             ("surface large", large & (comp is None))):
                    branches[k] += int(np.sum(m))
            sel = np.nonzero(counted)[0]
            if P.rr_intensity:
                e_col = e_col + 4 * EPS * (xs + 2 * dxmax)   # (a second leg starts from a rounded arrival point)
            column(idx[sel], (px + u[0] * s)[sel], (py + u[1] * s)[sel], e_col[sel], "ray column")
            if P.max_contrib is not None:
                mc = float(f32(P.max_contrib))
                decide(idx, np.abs(con - mc), e_con, "contribution limit")
                over = con > mc
                branches["capped above the limit"] += int(np.sum(over & capped))
                np.add.at(T["intensityExcess"], (cidx[over], d), con[over] - mc)
                np.add.at(Bd["intensityExcess"], (cidx[over], d), e_con[over])
                e_con = np.where(over, 0.0, e_con)
                con = np.where(over, mc, con)
            np.add.at(T["intensity"], (cidx, d, cj, ci), con)
            np.add.at(Bd["intensity"], (cidx, d, cj, ci), e_con)
            np.add.at(dep["intensity"], idx, con)

    def path_deposit(ph, cjs, cis, up_, wgt, ewt, lbin):
        """PATH: the photons `ph` end a flux tally in the columns (cjs, cis) with weight wgt: w L, w L^2 [path_add] or, by the bin of
        float(L), w and w L [bin_add, path_bin]; lbin: the path whose bin is taken (the photon's own, but for a control)"""
        Lh, eL = Lp[ph], e_L[ph]
        X["deposits"].append(np.array([ph, Lh, eL + EPS * Lh, wgt, np.full(len(ph), float(up_))]))
        b1, b2 = wgt * (ewt * Lh + eL), wgt * (ewt * Lh * Lh + 2.0 * Lh * eL)
        if extra == "paths":
            for key, val, bd in (("pathUp1" if up_ else "pathDown1", wgt * Lh, b1), ("pathUp2" if up_ else "pathDown2", wgt * Lh * Lh, b2)):
                np.add.at(T[key], (cjs, cis), val)
                np.add.at(Bd[key], (cjs, cis), bd)
                X["perPhoton"][key][ph] += val
            return
        xb = lbin.astype(f32).astype(f64)                                          # [bin_add: `const float x = (float)length`]
        bn = np.clip(np.searchsorted(edges, xb, side="right") - 1, 0, nbins)       # edges[b] <= x < edges[b + 1]; the overflow bin last
        m = np.where(bn < nbins, edges[np.minimum(bn + 1, nbins)] - lbin, np.inf)
        decide(ph, np.minimum(lbin - edges[bn], m), eL + EPS * lbin, "bin")       # (the path's own error and the conversion's rounding)
        for key, val, bd in (("binUp" if up_ else "binDown", wgt, wgt * ewt), ("binPathUp" if up_ else "binPathDown", wgt * Lh, b1)):
            np.add.at(T[key], bn, val)
            np.add.at(Bd[key], bn, bd)
            X["perPhoton"][key][ph] += val

    def track_pieces(g):
        """TRACK: the segments g cut by the planes of the grid (float64, periodic in x and y); each piece adds weight x length to the cell
        it lies in [trace_step_lazy LENGTH + track_add in photon_step; finish_arrival<true> + track_add in the event phase]"""
        m, sg, d = len(g["idx"]), g["s"], g["d"]
        goes_up = d[2] > 0

        def ragged(counts):
            counts = counts.astype(np.int64)
            return np.repeat(np.arange(m), counts), np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)

        at, off = ragged(np.abs(g["l1"] - g["l0"]))                                # the layer faces between the two layers
        k = np.where(goes_up[at], g["l0"][at] + 1 + off, g["l0"][at] - off)
        segs, ts, ncos = [at], [(ze[k] - g["z"][at]) / d[2, at]], [np.zeros(len(at))]
        for ax, (eds, org, width, nn, g0, g1, p0) in enumerate(((xe, x0, Lx, nx, g["gx0"], g["gx1"], g["x"]), (ye, y0, Ly, ny, g["gy0"], g["gy1"], g["y"]))):
            at, off = ragged(np.abs(g1 - g0))                                      # the side faces, counted through the periodic images
            G = np.where((g1 > g0)[at], g0[at] + 1 + off, g0[at] - off).astype(np.int64)
            face = org + (G // nn) * width + (eds[G % nn] - org)
            segs.append(at), ts.append((face - p0[at]) / d[ax, at]), ncos.append(np.abs(d[ax, at]))
        segs.append(np.arange(m)), ts.append(sg + 0.0), ncos.append(np.full(m, -1.0))   # (-1: the segment's end)
        at, nc = np.concatenate(segs), np.concatenate(ncos)
        t = np.clip(np.concatenate(ts), 0.0, sg[at])
        is_end = nc < 0
        o = np.lexsort((is_end, t, at))
        at, t, nc, is_end = at[o], t[o], nc[o], is_end[o]
        head = np.concatenate([[True], at[1:] != at[:-1]])
        t0 = np.where(head, 0.0, np.concatenate([[0.0], t[:-1]]))
        ell, tm = t - t0, 0.5 * (t + t0)
        px, py, pz = g["x"][at] + d[0, at] * tm, g["y"][at] + d[1, at] * tm, g["z"][at] + d[2, at] * tm
        ci_ = np.clip(np.searchsorted(xe, px - np.floor((px - x0) / Lx) * Lx, side="right") - 1, 0, nx - 1)
        cj_ = np.clip(np.searchsorted(ye, py - np.floor((py - y0) / Ly) * Ly, side="right") - 1, 0, ny - 1)
        lz_ = np.clip(np.searchsorted(ze, pz, side="right") - 1, 0, nz - 1)
        if variant == "piece credited to the cell after the step":
            nxt = np.where(is_end, np.arange(len(at)), np.minimum(np.arange(len(at)) + 1, len(at) - 1))
            ci_, cj_, lz_ = ci_[nxt], cj_[nxt], lz_[nxt]
        if variant == "arrival piece left out":
            ell = np.where(is_end & g["ev"][at], 0.0, ell)
        wt, ewt, adz_ = g["w"][at], g["e_w"][at], np.abs(d[2, at])
        side = nc > 0
        cs = np.cumsum(side) - side
        before = cs - cs[head][np.cumsum(head) - 1]                                # side faces crossed earlier in the segment
        # a piece's own length: one rounding [the quotient that `step` is, or finish_arrival's], the direction's error, the height's rounding at
        # every side face crossed before it [(side faces + 1) eps (|z|max + 2 dz) of the height: z is rounded only there], and the
        # along-path errors of the segment's two ends for the first and the last piece [e_s]
        e_l = EPS * ell + ell * g["e_dir"][at] / adz_ + before * EPS * (zs + 2 * dzmax) / adz_ + np.where(head, g["first"][at], 0.0) + np.where(is_end, g["last"][at], 0.0)
        bd = wt * (ewt * ell + e_l)
        val = wt * ell
        np.add.at(T["trackLayers"], lz_, val)
        np.add.at(Bd["trackLayers"], lz_, bd)
        # a side face: the position's error moves length from one cell to its neighbour, at most the shorter of the two pieces
        nxt_ell = np.concatenate([ell[1:], [0.0]])
        tr = np.where(side, wt * np.minimum(np.minimum(g["e_xy"][at] / np.maximum(nc, 1e-300), ell), nxt_ell), 0.0)
        bd = bd + tr + np.concatenate([[0.0], tr[:-1]])                            # (a side face is never a segment's last entry)
        np.add.at(T["tracks"], (lz_, cj_, ci_), val)
        np.add.at(Bd["tracks"], (lz_, cj_, ci_), bd)
        np.add.at(X["trackPieces"], (lz_, cj_, ci_), 1)
        np.add.at(X["perPhoton"]["tracks"], g["idx"][at], val)

    # ---- block 0: start position, first optical depth -------------------------------------------------------------------------
    all_ = np.arange(n)
    u = roles(all_, 0)
    x, y = x0 + u[0] * Lx, y0 + u[1] * Ly
    zstart = float(f32(P.ze[0] + f32(f32(f32(1.0) - f32(ULP)) * f32(P.ze[-1] - P.ze[0]))))
    assert zstart < ze[-1], "photons must start inside the domain (a thin elevated domain rounds the start to its top)"
    z = np.full(n, zstart)
    sun = direction(-abs(P.mu0), P.azimuth).astype(f64)
    dvec = np.repeat(sun[:, None], n, axis=1)
    w = np.ones(n)
    tau = -np.log(np.maximum(TINY, u[2]))
    blk = np.ones(n, np.int64)
    have = np.zeros(n, np.int64)
    cur = np.zeros((4, n))
    cnt["rngDraws"] += 3
    e_c, e_h, e_dir, e_w = np.zeros(n), np.full(n, 2 * EPS * xs), np.zeros(n), np.zeros(n)
    cix = np.clip(np.searchsorted(xe, x, side="right") - 1, 0, nx - 1).astype(f64)
    ciy = np.clip(np.searchsorted(ye, y, side="right") - 1, 0, ny - 1).astype(f64)
    lay = np.full(n, min(int(np.searchsorted(ze, zstart, side="right") - 1), nz - 1))
    alive = np.ones(n, bool)
    if extra == "levels" and variant != "new photon not counted":
        # a new photon is counted at the face of its start layer that lies behind it, downward, in its start column [part C, ST_NEW:
        # `down ? r.iz : r.iz - 1`, the column find_xy gave].  The start column is a decision: x0 + u (xMax - x0), one product, one sum
        ci_, cj_ = cix.astype(np.int64), ciy.astype(np.int64)
        decide(all_, np.minimum(np.minimum(x - xe[ci_], xe[ci_ + 1] - x), np.minimum(y - ye[cj_], ye[cj_ + 1] - y)), e_h, "start column")
        np.add.at(T["levelFluxDown"], (lay + 1, cj_, ci_), 1.0)
        X["perPhoton"]["levelFluxDown"][all_, lay + 1] += 1.0
    pfi_ev = None
    surface_z = float(f32(P.ze[0] + (np.spacing(np.abs(P.ze[0])) if P.ze[0] != 0 else f32(TINY))))   # z0 + spacing(z0)

    while alive.any():
        idx = np.nonzero(alive)[0]
        dz = dvec[2, idx]
        assert np.all(dz != 0.0)
        cnt["tracerCalls"][idx] += 1          # (one trace of the photon itself; the rays' are counted where they start)
        adz = np.abs(dz)
        up = dz > 0
        Cz = np.interp(z[idx], ze, cumz)
        Ct = Cz + np.where(up, 1.0, -1.0) * tau[idx] * adz
        top, bottom = up & (Ct >= cumz[-1]), ~up & (Ct <= 0.0)
        ev = ~(top | bottom)
        lnew = np.where(up, np.searchsorted(cumz, Ct, side="right") - 1, np.searchsorted(cumz, Ct, side="left") - 1)
        lnew = np.clip(lnew, 0, nz - 1)
        znew = np.where(top, ze[-1], np.where(bottom, ze[0], ze[lnew] + (np.minimum(np.maximum(Ct, cumz[lnew]), cumz[lnew + 1]) - cumz[lnew]) / np.where(ext[lnew] > 0, ext[lnew], 1.0)))
        s = (znew - z[idx]) / dz
        tau_tr = np.abs(np.interp(znew, ze, cumz) - Cz) / adz
        xu, yu = x[idx] + dvec[0, idx] * s, y[idx] + dvec[1, idx] * s
        # (the column first with the error of the step before: the faces crossed enter the bound)
        kx, ky = np.floor((xu - x0) / Lx), np.floor((yu - y0) / Ly)
        ci0 = np.clip(np.searchsorted(xe, xu - kx * Lx, side="right") - 1, 0, nx - 1)
        cj0 = np.clip(np.searchsorted(ye, yu - ky * Ly, side="right") - 1, 0, ny - 1)
        nxy = np.abs(kx * nx + ci0 - cix[idx]) + np.abs(ky * ny + cj0 - ciy[idx])
        steps = np.abs(lnew - lay[idx]) + nxy + 1
        # (in the vertical optical-depth coordinate C: the start's error, the target's, the steps' roundings, the direction's)
        e_ct = e_c[idx] + adz * (2 * ULP * tau[idx] + 3 * EPS * steps * tau_tr) + extmax * (nxy + 1) * EPS * (zs + 2 * dzmax) + tau_tr * e_dir[idx]
        m_face = np.where(ev, np.minimum(Ct - cumz[lnew], cumz[lnew + 1] - Ct), np.where(top, Ct - cumz[-1], -Ct))
        decide(idx, m_face, e_ct, "top / bottom / layer")
        ext_new, ext_old = np.where(ext[lnew] > 0, ext[lnew], 1.0), np.where(ext[lay[idx]] > 0, ext[lay[idx]], 1.0)
        e_cn = np.where(ev, e_ct + 4 * EPS * zs * ext_new, 0.0)
        e_s = (e_cn / ext_new + e_c[idx] / ext_old) / adz + np.abs(s) * e_dir[idx] / adz
        e_xy = e_h[idx] + np.abs(s) * e_dir[idx] + np.maximum(np.abs(dvec[0, idx]), np.abs(dvec[1, idx])) * e_s + steps * EPS * (xs + 2 * dxmax)
        xw, yw, ci, cj, _ = column(idx, xu, yu, e_xy, "column")
        sabs = np.abs(s)
        L_before = Lp[idx].copy()
        if path_kind:
            # the path grows by the pieces the tracer steps [photon_step: `pathLen += (double)len`; the event phase: `pathLen +=
            # (double)part`]: the segment's along-path error, and one float32 rounding per voxel-step piece and for the arrival piece
            Lp[idx] += sabs
            e_L[idx] += e_s + steps * EPS * sabs
        if extra == "levels":
            # a segment from layer a to layer b adds its weight to levelFluxUp[a .. b - 1] going up, to levelFluxDown[b .. a - 1] going
            # down [part A: tally_level_crossings with izFrom, and izTo = nz + 1 at the top, 0 on the surface]
            a_, b_ = lay[idx] + 1, np.where(top, nz + 1, np.where(bottom, 0, lnew + 1))
            sh = 1 if variant == "downward range shifted by one level" else 0
            dh = np.maximum(np.abs(dvec[0, idx]), np.abs(dvec[1, idx]))
            for k in range(nz + 1):
                for key, hit, ends in (("levelFluxUp", up & (a_ <= k) & (k <= b_ - 1), top & (k == nz)),
                                       ("levelFluxDown", ~up & (b_ + sh <= k) & (k <= a_ - 1 + sh), bottom & (k == 0))):
                    h = np.nonzero(hit)[0]
                    if not len(h):
                        continue
                    li, lj = ci[h].copy(), cj[h].copy()         # the level a segment ends on takes the arrival's own column
                    far = ~ends[h]
                    q = h[far]
                    if len(q) and variant != "crossing counted in the arrival column":
                        # every other level: the column of the point where the straight segment meets ze[k], which the kernel extrapolates
                        # BACK from the arrival in float32 [tally_level_crossings]: back = (z - zE[k]) / dz (a difference, a quotient),
                        # cx = x - dx * back (a product, a difference), cx - floorf((cx - x0) / widthX) * widthX (a difference, a
                        # quotient, a product, a difference); the clamp rounds nothing
                        tk = (ze[k] - z[idx[q]]) / dz[q]
                        back = s[q] - tk
                        hb = dh[q] * np.abs(back)
                        e_lc = e_xy[q] + np.abs(back) * e_dir[idx[q]] + EPS * (3 * hb + 4 * (xs + hb) + xs)
                        _, _, pi_, pj_, _ = column(idx[q], x[idx[q]] + dvec[0, idx[q]] * tk, y[idx[q]] + dvec[1, idx[q]] * tk, e_lc, "level column")
                        li[far], lj[far] = pi_, pj_
                    np.add.at(T[key], (k, lj, li), w[idx[h]])
                    np.add.at(Bd[key], (k, lj, li), w[idx[h]] * e_w[idx[h]])
                    X["perPhoton"][key][idx[h], k] += w[idx[h]]
        if extra == "tracks":
            trk = dict(idx=idx, x=x[idx].copy(), y=y[idx].copy(), z=z[idx].copy(), d=dvec[:, idx].copy(), s=sabs, l0=lay[idx].copy(), l1=lnew,
                       gx0=cix[idx].copy(), gy0=ciy[idx].copy(), gx1=kx * nx + ci0, gy1=ky * ny + cj0, ev=ev, w=w[idx].copy(), e_w=e_w[idx].copy(),
                       e_dir=e_dir[idx].copy(), e_xy=e_xy, first=e_c[idx] / ext_old / adz, last=e_cn / ext_new / adz)
            X["perPhoton"]["wS"][idx] += w[idx] * sabs
        x[idx], y[idx], z[idx] = xw, yw, znew
        cix[idx], ciy[idx], lay[idx] = ci, cj, lnew
        e_c[idx], e_h[idx] = e_cn, e_xy

        # ---- exits through the top ------------------------------------------------------------------------------------------
        t = idx[top]
        np.add.at(T["fluxUp"], (cj[top], ci[top]), w[t])
        np.add.at(Bd["fluxUp"], (cj[top], ci[top]), w[t] * e_w[t])
        dep["fluxUp"][t] += w[t]
        cnt["exitsTop"][t] += 1
        if path_kind and len(t):   # [part A: bin_add / path_add beside tally.boundary, the same column]
            if variant == "last segment left out of L":
                Lp[t] = L_before[top]
            path_deposit(t, cj[top], ci[top], True, w[t], e_w[t], L_before[top] if variant == "bin of L before the last segment" else Lp[t])
        fate[t], wfin[t], alive[t] = 0, w[t], False

        # ---- the surface ----------------------------------------------------------------------------------------------------
        b = idx[bottom]
        if len(b):
            np.add.at(T["fluxDown"], (cj[bottom], ci[bottom]), w[b])
            np.add.at(Bd["fluxDown"], (cj[bottom], ci[bottom]), w[b] * e_w[b])
            dep["fluxDown"][b] += w[b]
            cnt["surfaceHits"][b] += 1
            if path_kind:   # the weight BEFORE the reflection, the path up to here [part A for a black surface; part C beside tally.down]
                if variant == "last segment left out of L":
                    Lp[b] = L_before[bottom]
                wb = w[b] * alb if variant == "surface tally with the weight after the reflection" else w[b]
                path_deposit(b, cj[bottom], ci[bottom], False, wb, e_w[b], L_before[bottom] if variant == "bin of L before the last segment" else Lp[b])
            fate[b], wfin[b] = 1, w[b]
            if black:
                alive[b] = False
            else:
                u = roles(b, blk[b])
                blk[b] += 1
                cnt["rngDraws"][b] += 2
                order[b] += 1
                assert np.all(u[0] > 0.0), "a reflection's deviate of exactly 0 (the retry) is not modelled"
                mu = np.sqrt(u[0].astype(f32)).astype(f32)                      # exact_sqrt
                sinT = np.sqrt((f32(1.0) - (mu * mu).astype(f32)).astype(f32)).astype(f32).astype(f64)
                turn = u[0] if variant == "azimuth from first" else u[1]
                w[b] = w[b] * alb
                e_w[b] += EPS
                dead = w[b] <= TINY
                alive[b[dead]] = False
                g = b[~dead]
                sg, tg = sinT[~dead], turn[~dead]
                dvec[:, g] = np.array([sg * np.cos(2 * np.pi * tg), sg * np.sin(2 * np.pi * tg), mu[~dead].astype(f64)])
                e_dir[g] = SINCOS * np.sqrt(2.0) * sg + 2 * EPS
                z[g] = surface_z
                lay[g] = 0
                if variant == "path restarts at a reflection":
                    Lp[g], e_L[g] = 0.0, 0.0
                if extra == "levels" and variant != "reflected photon not counted":
                    # levelFluxUp[0]: the reflected weight, in the column where it was reflected [part C: `add_global(... + c2, w)`
                    # behind `w = w * Pe.albedo`, only for a photon that goes on]
                    gj, gi = cj[bottom][~dead], ci[bottom][~dead]
                    np.add.at(T["levelFluxUp"], (0, gj, gi), w[g])
                    np.add.at(Bd["levelFluxUp"], (0, gj, gi), w[g] * e_w[g])
                    X["perPhoton"]["levelFluxUp"][g, 0] += w[g]
                if nd:
                    radiance(g, None, x[g], y[g], z[g], None, w[g], e_c[g], e_h[g], e_dir[g], e_w[g], order[g])
                tau[g] = -np.log(np.maximum(TINY, u[2][~dead]))
                cnt["rngDraws"][g] += 1

        # ---- scatterings ----------------------------------------------------------------------------------------------------
        e = idx[ev]
        if len(e):
            le, cie, cje = lnew[ev], ci[ev], cj[ev]
            u = roles(e, blk[e])
            blk[e] += 1
            order[e] += 1
            cnt["scatterings"][e] += 1
            comp = np.ones(len(e), np.int64)
            if ncomp > 1:
                need = have[e] == 0
                if need.any():
                    r = e[need]
                    words = philox(lo[r], hi[r], blk[r], 0, k0, k1)
                    cur[:, r] = np.array([unit(v) for v in words])
                    blk[r] += 1
                    have[r] = 4
                rc = cur[4 - have[e], e]
                have[e] -= 1
                cnt["rngDraws"][e] += 1
                for k in range(ncomp - 1):
                    comp += rc >= frac[k, le]
                    decide(e, np.abs(rc - frac[k, le]) + np.where(rc == frac[k, le], 1.0, 0.0), np.zeros(len(e)), "component")
            om = P.ssa[comp - 1, le].astype(f64)
            pfi_ev = np.maximum(P.pfi[comp - 1, le], 1)
            absorbing = om < 1.0
            inc = np.where(absorbing, w[e] * (1.0 - om), 0.0)
            np.add.at(T["volumeAbsorption"], (le, cje, cie), inc)
            np.add.at(Bd["volumeAbsorption"], (le, cje, cie), inc * (e_w[e] + 2 * EPS))
            dep["volumeAbsorption"][e] += inc
            if extra == "levels":
                X["perPhoton"]["absLayer"][e, le] += inc
            w[e] = np.where(absorbing, w[e] * om, w[e])
            if variant == "weight after the scattering":
                trk["w"][ev] = w[e]
            e_w[e] += np.where(absorbing, EPS, 0.0)
            if nd:
                radiance(e, comp, x[e], y[e], z[e], dvec[:, e], w[e], e_c[e], e_h[e], e_dir[e], e_w[e], order[e])
            if P.roulette:
                decide(e, np.abs(w[e] - 0.5), w[e] * e_w[e], "roulette")
                play = w[e] < 0.5
                cnt["roulette"][e[play]] += 1
                cnt["rngDraws"][e[play]] += 1
                decide(e[play], np.abs(u[3][play] - w[e][play]), (w[e] * e_w[e])[play], "roulette")
                lost = play & (u[3] >= w[e])
                w[e] = np.where(play, np.where(lost, 0.0, 1.0), w[e])
                e_w[e] = np.where(play, 0.0, e_w[e])
            dead = w[e] <= TINY
            fate[e[dead]], wfin[e[dead]] = 2, 0.0
            alive[e[dead]] = False
            g, keep = e[~dead], ~dead
            if len(g):
                # scattering_cosine<false>, float32 operation by operation
                # (refined_rcp(n) is v_rcp with one Newton step: the correctly rounded 1 / n or a neighbour.  The cosine is formed with
                # all three; where they do not agree to the bit the kernel's may be either, one ulp apart)
                r32 = u[0][keep].astype(f32)
                cosS, unsure = np.zeros(len(g), f32), np.zeros(len(g), bool)
                for c in range(1, ncomp + 1):
                    sel = comp[keep] == c
                    if not sel.any():
                        continue
                    tab = cosT[c - 1]
                    nI = tab.shape[1]
                    row = pfi_ev[keep][sel] - 1
                    rr = r32[sel]
                    k = (rr * f32(nI)).astype(f32).astype(np.int64) + 1
                    inside = k < nI
                    kk = np.minimum(k, nI - 1)
                    shift = 1 if variant == "table interval k + 1" else 0
                    a, bb = tab[row, np.minimum(kk - 1 + shift, nI - 1)], tab[row, np.minimum(kk + shift, nI - 1)]
                    rcp = f32(f32(1.0) / f32(nI))
                    vals = []
                    for rn in (rcp, np.nextafter(rcp, f32(0)), np.nextafter(rcp, f32(1))):
                        left = (rr - ((kk - 1).astype(f32) * rn).astype(f32)).astype(f32)
                        val = (((f32(1.0) - left).astype(f32) * a).astype(f32) + (left * bb).astype(f32)).astype(f32)
                        vals.append(np.where(inside, val, tab[row, nI - 1]))
                    cosS[sel] = vals[0]
                    unsure[sel] = (vals[1] != vals[0]) | (vals[2] != vals[0])
                ysq = (f32(1.0) - (cosS * cosS).astype(f32)).astype(f32).astype(f64)
                sinT = np.sqrt(np.maximum(ysq, 0.0))
                cS = cosS.astype(f64)
                turn = (u[0] if variant == "azimuth from first" else u[1])[keep]
                sold = dvec[:, g]
                decide(g, np.abs(sold[2]), e_dir[g], "frame")
                snew = rotate(sold, cS, sinT, turn)
                # the rotation's own gain at this event: finite differences along two tangents of the old direction
                h = 1e-8
                ref = np.where(np.abs(sold[0]) < 0.6, 1.0, 0.0)
                axis = np.array([ref, 1.0 - ref, np.zeros(len(g))])
                t1 = np.cross(sold.T, axis.T).T
                t1 /= np.linalg.norm(t1, axis=0)
                t2 = np.cross(sold.T, t1.T).T
                ja, jb = (rotate(sold + h * t1, cS, sinT, turn) - snew) / h, (rotate(sold + h * t2, cS, sinT, turn) - snew) / h
                aa, bb_, ab = (ja * ja).sum(0), (jb * jb).sum(0), (ja * jb).sum(0)
                gain = np.sqrt(0.5 * (aa + bb_ + np.sqrt((aa - bb_) ** 2 + 4 * ab * ab)))   # largest singular value of (ja jb)
                e_cos = np.where(unsure, np.minimum(ULP / np.maximum(sinT, 1e-300), np.sqrt(2 * ULP)), 0.0)
                e_dir[g] = gain * e_dir[g] + e_cos + (SINCOS * np.sqrt(2.0) + 3 * ULP) * sinT + 10 * EPS
                dvec[:, g] = snew
                tau[g] = -np.log(np.maximum(TINY, u[2][keep]))
                cnt["rngDraws"][g] += 3
        if extra == "tracks":
            track_pieces(trk)

    T["fluxAbsorbed"] = T["volumeAbsorption"].sum(0)
    Bd["fluxAbsorbed"] = Bd["volumeAbsorption"].sum(0)
    dep["fluxAbsorbed"] = dep["volumeAbsorption"]
    if nd == 0:
        for k in ("intensity", "intensityExcess"):
            T.pop(k), Bd.pop(k)
    counters = {k: int(v.sum()) for k, v in cnt.items()}
    counters.update(photons=n, dropped=0)
    # what a fragile photon may carry into an entry other than the model's: its weight never exceeds 1, so 1 per tally it can make
    # plus what the model itself has it deposit; a radiance contribution is at most max P / (4 pi min |mu_d|) (or the limit, or 1 / pi)
    caps = {k: 1.0 + dep[k] for k in ("fluxUp", "fluxDown", "fluxAbsorbed", "volumeAbsorption")}
    if nd:
        cmax = max(max(float(t.max()) for t in P.fwd + P.fwd_orig) / (4 * np.pi * float(np.abs(P.dirs[:, 2]).min())), 1 / np.pi)
        if P.max_contrib is not None:
            cmax = min(cmax, float(P.max_contrib))
        if P.rr_intensity:
            cmax = max(cmax, zeta / np.pi)
        caps["intensity"] = dep["intensity"] + (order + 1) * cmax
        caps["intensityExcess"] = caps["intensity"]
    per = dict(fate=fate, order=order, weight=wfin, fragile=fragile, why=why, **{"n_" + k: v for k, v in cnt.items()})
    exact_zero = {}
    if nd and P.rr_intensity:   # only an exit through the top counts: no float32 decision stands between a downward direction and 0
        for k in ("intensity", "intensityExcess"):
            exact_zero[k] = np.zeros(T[k].shape, bool)
            exact_zero[k][:, P.dirs[:, 2] < 0] = True
    if path_kind:
        X["path"], X["pathError"] = Lp, e_L     # every photon's path at its end, and the model's bound on it
        # every tally of a path, one column each: photon (its index in this run), L, the bound on float(L), weight, 1 up / 0 down
        X["deposits"] = np.concatenate(X["deposits"], axis=1) if X["deposits"] else np.zeros((5, 0))
    return Result(n, T, Bd, counters, per, caps, branches, X, exact_zero)


def _rowwise(rows, theta):
    """lookup_phase_fast with one table row per angle"""
    nf = rows.shape[1]
    rcp = float(f32(f32(nf - 1) * f32(f32(1.0) / PI32)))
    pos = theta * rcp
    k = pos.astype(np.int64) + 1
    inside = k < nf
    kk = np.minimum(k, nf - 1)
    fr = pos - (kk - 1)
    i = np.arange(len(theta))
    return np.where(inside, (1.0 - fr) * rows[i, kk - 1] + fr * rows[i, kk], rows[i, nf - 1]), pos


def clean_range(model, start=0):
    """(first, count) of the longest run of consecutive photons of a run (from its photon `start` on) none of which is fragile: launched
    on its own, that range must give the model's counters exactly and its tallies within the float32 bound alone"""
    frag = np.nonzero(model.per_photon["fragile"])[0]
    edges = np.concatenate([[start - 1], frag[frag >= start], [model.n]])
    k = int(np.argmax(np.diff(edges)))
    return int(edges[k] + 1), int(edges[k + 1] - edges[k] - 1)


def clean_runs(model, start=0, least=1):
    """[(first, count)] of ALL maximal runs of at least `least` consecutive photons of a run (from its photon `start` on) none of which is
    fragile, in order.  The diagnostic tallies are compared over exactly these photons: a path has no upper limit, so nothing caps what
    a fragile photon may carry into a path sum, a bin or a cell's track length"""
    frag = np.nonzero(model.per_photon["fragile"])[0]
    cuts = np.concatenate([[start - 1], frag[frag >= start], [model.n]])
    return [(int(a + 1), int(b - a - 1)) for a, b in zip(cuts[:-1], cuts[1:]) if b - a - 1 >= max(least, 1)]


def run_ids(runs, offset=0):
    """the photon numbers of the runs [(first, count)], as `run(..., ids=...)` takes them"""
    return np.concatenate([np.uint64(offset) + np.uint64(a) + np.arange(c, dtype=np.uint64) for a, c in runs])


COUNTERS_EXACT = ("photons", "dropped")
COUNTERS_FRAGILE = ("scatterings", "surfaceHits", "exitsTop", "roulette", "rngDraws", "raysSkipped", "tracerCalls")


def compare_counters(models, counters, names=COUNTERS_EXACT + COUNTERS_FRAGILE):
    """counters (of one run, or summed over several) against the models' sums; the fragile photons' own counts are the allowance"""
    miss = []
    for k in names:
        want = sum(m.counters[k] for m in models)
        allow = 0 if k in COUNTERS_EXACT else sum(int(m.per_photon["n_" + k][m.per_photon["fragile"]].sum()) for m in models)
        if abs(int(counters[k]) - want) > allow:
            miss.append((k, int(counters[k]), want, allow))
    return miss


def compare(model, tallies, counters, counter_names=COUNTERS_EXACT + COUNTERS_FRAGILE):
    """Hold another run's raw tallies (sums over photons, shaped as the model's) and counters against the model's.  Returns
    (list of misses, {field: largest difference / its tolerance}); the caller asserts that the list is empty."""
    frag = model.per_photon["fragile"]
    miss, worst = compare_counters([model], counters, counter_names), {}
    for k, want in model.tallies.items():
        got = np.asarray(tallies[k], f64).reshape(want.shape)
        if k in model.caps:
            slack = float(model.caps[k][frag].sum())
        else:   # a diagnostic field: a path has no upper limit, so a fragile photon has no cap -- such a field is compared over photons none of which is fragile
            assert not frag.any(), (k, "a diagnostic tally is compared only over photons that are not fragile")
            slack = 0.0
        tol = model.bounds[k] + slack
        if k in model.exact_zero:
            assert not want[model.exact_zero[k]].any()
            tol = np.where(model.exact_zero[k], 0.0, tol)
        diff = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(diff > 0, diff / np.where(tol > 0, tol, TINY), 0.0)
        worst[k] = float(ratio.max())
        if worst[k] > 1.0:
            at = np.unravel_index(int(ratio.argmax()), ratio.shape)
            miss.append((k, at, float(got[at]), float(want[at]), float(tol[at])))
    return miss, worst


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------
# name -> dict(domain=..., tables=[per component (g of each table entry)], params) ; domains are 4 x 3 columns over layers with gaps
def _layers(nz, z0, regular=True, seed=1):
    if regular:
        return (f32(z0) + f32(3.5) * np.arange(nz + 1, dtype=f32)).astype(f32)
    rng = np.random.default_rng(seed)
    return (f32(z0) + np.concatenate([[0.0], np.cumsum(rng.uniform(2, 5, nz))])).astype(f32)


_XE, _YE = f32(120.0) * np.arange(5, dtype=f32), f32(150.0) * np.arange(4, dtype=f32)
_XI, _YI = np.array([0, 70, 190, 300, 480], f32), np.array([0, 130, 210, 450], f32)


def _case(ext, ssa, pfi, gs, ze, xe=_XE, ye=_YE, n=20_000, **kw):
    return dict(xe=xe, ye=ye, ze=ze, ext=np.atleast_2d(np.asarray(ext, f32)), ssa=np.atleast_2d(np.asarray(ssa, f32)),
                pfi=np.atleast_2d(np.asarray(pfi, np.int64)), gs=gs, n=n, params=kw)


def _cases():
    C = {}
    e8 = np.array([0.04, 0.0, 0.06, 0.02, 0.0, 0.0, 0.05, 0.03], f32)      # optical depth 0.7 in 8 layers of 3.5 m, three of them empty:
    # free paths are short beside the columns (120 m and more), so few photons come within their own error of a column's side
    on = (e8 > 0)
    C["a common"] = _case(e8, on * f32(1.0), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.3)
    C["a absorbing"] = _case(e8, on * f32(0.9), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.3)
    ssa_b = np.where(on, np.array([0.99, 0, 0.8, 0.95, 0, 0, 0.6, 1.0], f32), 0)
    C["b records"] = _case(e8, ssa_b, on * np.array([1, 0, 2, 1, 0, 0, 2, 2]), [(0.85, 0.6)], _layers(8, 6.0), albedo=0.3)
    gas = np.linspace(0.03, 0.02, 8, dtype=f32)
    C["c two"] = _case([e8, gas], [on * f32(0.98), np.full(8, f32(0.6))], [on * np.array([1, 0, 2, 1, 0, 0, 2, 1]), np.ones(8)],
                       [(0.85, 0.6), (0.0,)], _layers(8, 0.0, False), albedo=0.3)
    aer = np.array([0.02, 0.02, 0.01, 0, 0, 0, 0, 0], f32)
    C["d three"] = _case([e8, aer, gas], [on * f32(0.98), (aer > 0) * f32(0.92), np.full(8, f32(0.6))],
                         [on * 1, (aer > 0) * 1, np.ones(8)], [(0.85,), (0.7,), (0.0,)], _layers(8, 0.0, False), albedo=0.3)
    C["e irregular"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), xe=_XI, ye=_YI, albedo=0.3)
    C["f no roulette"] = _case(e8, on * f32(0.4), on * 1, [(0.6,)], _layers(8, 6.0), albedo=0.3, roulette=False)
    C["f roulette"] = _case(e8, on * f32(0.4), on * 1, [(0.6,)], _layers(8, 6.0), albedo=0.3, roulette=True)
    C["g black"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.0)
    C["g white"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), albedo=1.0)
    C["h one up"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.3, mus=[0.8], phis=[30.0], n=10_000)
    C["h one down"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.3, mus=[-0.6], phis=[200.0], n=10_000)
    C["h three"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.3, mus=[1.0, 0.7, -0.8], phis=[0.0, 120.0, 250.0], n=10_000)
    C["h three two components"] = _case([e8, gas], [on * f32(0.98), np.full(8, f32(0.6))], [on * np.array([1, 0, 2, 1, 0, 0, 2, 1]), np.ones(8)],
                                        [(0.85, 0.6), (0.0,)], _layers(8, 6.0), albedo=0.3, mus=[1.0, 0.8, -0.7], phis=[0.0, 120.0, 250.0], n=10_000)
    C["h hybrid"] = _case(e8, on * f32(0.95), on * 1, [(0.95,)], _layers(8, 6.0), albedo=0.3, mus=[0.9], phis=[10.0], hybrid=1, n=10_000)
    C["h limit"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), albedo=0.3, mus=[0.9, 0.4], phis=[10.0, 200.0], limit=0.5, n=10_000)
    # ... and with the local estimate's own roulette (make_ray's tail, the service phase's stages): the same media and directions
    rr = dict(albedo=0.3, rr_intensity=True, n=10_000)
    C["r one up"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), mus=[0.8], phis=[30.0], **rr)
    C["r one down"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), mus=[-0.6], phis=[200.0], **rr)
    C["r three"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), mus=[1.0, 0.7, -0.8], phis=[0.0, 120.0, 250.0], **rr)
    C["r three two components"] = _case([e8, gas], [on * f32(0.98), np.full(8, f32(0.6))], [on * np.array([1, 0, 2, 1, 0, 0, 2, 1]), np.ones(8)],
                                        [(0.85, 0.6), (0.0,)], _layers(8, 6.0), mus=[1.0, 0.8, -0.7], phis=[0.0, 120.0, 250.0], **rr)
    C["r hybrid"] = _case(e8, on * f32(0.95), on * 1, [(0.95,)], _layers(8, 6.0), mus=[0.9], phis=[10.0], hybrid=1, **rr)
    # (a limit below zetaMin / pi = 0.095: capped values of the heavier photons exceed it, and so does every large contribution)
    C["r limit"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), mus=[0.9, 0.4], phis=[10.0, 200.0], limit=0.08, **rr)
    # (zetaMin above 1: the surface's pi norm = 1 is a small contribution)
    C["r zeta"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), mus=[0.6, -0.9], phis=[40.0, 300.0], zeta_min=1.5, **rr)
    # (columns a hundred times as wide: hardly a photon or a ray comes within its own error of a column's side, so the WHOLE case allows
    # next to nothing beyond the float32 bound -- the case on which the controls of tests/test_stream_model_cpu.py are seen on a whole case)
    C["r wide"] = _case(e8, on * f32(0.95), on * 1, [(0.85,)], _layers(8, 6.0), xe=f32(100.0) * _XE, ye=f32(100.0) * _YE,
                        mus=[1.0, 0.4, -0.8], phis=[0.0, 120.0, 250.0], limit=0.08, **rr)
    return C


CASES = _cases()
SUN = (0.7, 25.0)
SEED = (23, 4)
FRAGILE_CAP = 0.005
# A fused launch hands out every batch's photons from 0 on, so its run without a fragile photon has to begin there: with this key the
# first FUSED_CLEAN_N photons of batches 0, 1 and 2 (key (seed0, seed1 + batch)) of `r one up` and `r three` hold none -- the first ones
# are photons 765, 787 and 1335 (found by running the model over first key words 1 .. 120; asserted in tests/test_stream_model_cpu.py)
FUSED_CLEAN_SEED, FUSED_CLEAN_N, FUSED_CLEAN_CASES = (3, 4), 750, ("r one up", "r three")


def problem(case, inverse, forward=None, forward_orig=None, dirs=None, extra=None, bin_edges=None):
    """the model's problem for a shared case, with the tables (and directions) the host hands to the device"""
    p = case["params"]
    return Problem(case["xe"], case["ye"], case["ze"], case["ext"], case["ssa"], case["pfi"], inverse, mu0=SUN[0], azimuth=SUN[1],
                   albedo=p["albedo"], roulette=p.get("roulette", True), dirs=dirs, fwd=forward, fwd_orig=forward_orig,
                   hybrid=bool(p.get("hybrid")), orders_orig=int(p.get("hybrid", 0)), max_contrib=p.get("limit"),
                   rr_intensity=bool(p.get("rr_intensity", False)), zeta_min=p.get("zeta_min", 0.3), extra=extra, bin_edges=bin_edges)


# ---- the diagnostic tallies' cases --------------------------------------------------------------------------------------------------
# The flux cases (the diagnostics refuse radiance directions) at their own sizes: 20 000 photons, 4 x 3 columns, 8 layers.  A case whose
# share of fragile photons with the kind's new decisions (start column, level column, bin) would exceed FRAGILE_CAP, or whose track
# bounds would exceed TRACK_RESOLUTION, is RESHAPED for that kind as `r wide` is: the same medium under columns a hundred times as wide
# (conditions on the inputs, asserted in tests/test_stream_model_cpu.py; the bound and the cap stay)
KINDS = EXTRAS[1:]
DIAGNOSTIC_CASES = ("a absorbing", "b records", "c two", "e irregular", "f no roulette", "g black", "g white")
DIAGNOSTIC_WIDE = {"levels": ("e irregular", "f no roulette", "g white"), "tracks": ("b records", "g white"), "paths": (),
                   "bins": ("c two", "e irregular", "f no roulette", "g white")}
# ... and `g white` runs its track lengths over photons 60 000 .. 79 999: the columns do not reshape what misses the resolution there.  A
# white surface sends photons up again and again, some of them within a few 1e-5 of the horizontal -- just beyond 4 bounds of the
# "frame" decision --, and one such photon's 28 m inside one cell, uncertain by the relative error e_dir / |dz| of its slant, is a
# bound of 1.6e-3 of that cell's entry on its own (photons 0 .. 19 999: photon 14 185, |dz| 1.4e-5, e_dir 3.3e-6).  Of the twelve ranges
# of 20 000 photons from 0 on, this is the first whose worst cell is below half the resolution (4.5e-4)
DIAGNOSTIC_FIRST = {("tracks", "g white"): 60_000}
TRACK_RESOLUTION = 1e-3     # summed bound / entry in every cell with TRACK_PIECES pieces: what the statistical tests resolve already
TRACK_PIECES = 1000
# The histogram's edges: 0, then a geometric progression (first edge, ratio, bins), chosen on the CPU per case so that the overflow bin
# holds something but under 1 % of the weight, 20 bins hold 100 photons each and the bin decision leaves the fragile share within the
# cap.  One progression does not serve every case: the long paths of `f no roulette` and `g white` (no roulette; a white surface) carry
# the largest path errors and want wide bins, the 20 000 single tallies of `g black` fill 20 bins only where the bins are narrow
BIN_EDGES = {"a common": (20.0, 1.06, 50), "a absorbing": (20.0, 1.06, 50), "b records": (20.0, 1.06, 50), "c two": (20.0, 1.06, 50), "e irregular": (20.0, 1.06, 50),
             "f no roulette": (10.0, 1.15, 24), "g black": (20.0, 1.04, 60), "g white": (10.0, 1.15, 30)}


def bin_edges(name):
    first, ratio, nbins = BIN_EDGES[name]
    return np.concatenate([[0.0], first * f64(ratio) ** np.arange(nbins)]).astype(f32)


def diagnostic_case(name, kind):
    """the shared case `name` as the diagnostic kind runs it: its own, or under columns a hundred times as wide (DIAGNOSTIC_WIDE)"""
    c = dict(CASES[name])
    if name in DIAGNOSTIC_WIDE[kind]:
        c["xe"], c["ye"] = (f32(100.0) * c["xe"]).astype(f32), (f32(100.0) * c["ye"]).astype(f32)
    return c


def unscattered_path(P):
    """the path of a photon that reaches the surface without an event: (zstart - ze[0]) / |mu0| with the host's direction"""
    zstart = float(f32(P.ze[0] + f32(f32(f32(1.0) - f32(ULP)) * f32(P.ze[-1] - P.ze[0]))))
    return (zstart - float(P.ze[0])) / abs(float(direction(-abs(P.mu0), P.azimuth)[2]))


def case_directions(case):
    p = case["params"]
    return None if "mus" not in p else np.array([direction(m, ph) for m, ph in zip(p["mus"], p["phis"])], f32)


# fragile photons / photons of every shared case at its size, seed SEED, photons from 0 (python -m tests.stream_model prints them)
FRAGILE_SHARES = {
    'a common': 0.0019,
    'a absorbing': 0.0013,
    'b records': 0.00135,
    'c two': 0.00245,
    'd three': 0.0028,
    'e irregular': 0.00225,
    'f no roulette': 0.00455,
    'f roulette': 0.00025,
    'g black': 0.0008,
    'g white': 0.00435,
    'h one up': 0.0027,
    'h one down': 0.0029,
    'h three': 0.0033,
    'h three two components': 0.0047,
    'h hybrid': 0.0032,
    'h limit': 0.0031,
    'r one up': 0.0021,
    'r one down': 0.0014,
    'r three': 0.0023,
    'r three two components': 0.0023,
    'r hybrid': 0.0024,
    'r limit': 0.0021,
    'r zeta': 0.0015,
    'r wide': 0.001,
}

# ... and of every diagnostic case and kind, the kind's own decisions among the reasons, at the shapes and photons S.diagnostic_case,
# BIN_EDGES and DIAGNOSTIC_FIRST give (`a common`: the histogram's exact-sum case alone)
DIAGNOSTIC_SHARES = {
    'levels': {'a absorbing': 0.0035, 'b records': 0.0028, 'c two': 0.0045, 'e irregular': 0.00125, 'f no roulette': 0.002, 'g black': 0.0022, 'g white': 0.00215},
    'tracks': {'a absorbing': 0.0013, 'b records': 0.00055, 'c two': 0.00245, 'e irregular': 0.00225, 'f no roulette': 0.00455, 'g black': 0.0008, 'g white': 0.00095},
    'paths': {'a absorbing': 0.0013, 'b records': 0.00135, 'c two': 0.00245, 'e irregular': 0.00225, 'f no roulette': 0.00455, 'g black': 0.0008, 'g white': 0.00435},
    'bins': {'a common': 0.0046, 'a absorbing': 0.0031, 'b records': 0.00385, 'c two': 0.00445, 'e irregular': 0.0031, 'f no roulette': 0.0042, 'g black': 0.00315,
             'g white': 0.0038},
}

if __name__ == "__main__":
    from tests.test_stream_model_cpu import model_for

    for name in CASES:
        r = model_for(name)
        print(f"{name:26s} n {r.n:6d} fragile {r.fragile_share:.5f} {r.per_photon['why']} mean order {r.per_photon['order'].mean():.2f}")
        if CASES[name]["params"].get("rr_intensity"):
            first, count = clean_range(r)
            print(f"{'':26s} rays {r.branches}\n{'':26s} clean run {first} + {count}: {model_for(name, first=first, n=count).branches}")
    from tests.test_stream_model_cpu import diagnostic_model

    for kind in KINDS:
        for name in DIAGNOSTIC_CASES + (("a common",) if kind == "bins" else ()):
            r = diagnostic_model(name, kind)
            print(f"{kind:7s} {name:14s} {'wide' if name in DIAGNOSTIC_WIDE[kind] else 'own ':4s} fragile {r.fragile_share:.5f} {r.per_photon['why']}")

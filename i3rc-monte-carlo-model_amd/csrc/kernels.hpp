// gfx950 kernels of the I3RC photon tracer.
//
// Mapping (MI355X-first, not a port of the scalar Fortran loop nest):
//   * one photon per LANE, 64 photons in flight per wavefront, persistent waves: a lane that loses its photon
//     (exit, absorption, roulette, tracer drop) gets the next photon index from the wave's reservoir, which is
//     refilled from a device-wide counter with one returning atomic per <= 256 photons;
//   * the reference's three nested data-dependent loops (photon / order of scattering / voxel step,
//     computeRT :452-691 + accumulateExtinctionAlongPath :1690-1806) are flattened into a lane state machine with
//     ballot-gated phases: a VOXEL-STEP phase executed by the lanes that are tracing and an EVENT phase (exit tallies,
//     next photon, one Philox block for the whole wave, scatter / surface / new photon, new optical depth) that runs
//     when enough lanes wait for it;
//   * radiances: an event pushes ONE record into its wave's ray queue (a ring in LDS) and the photon goes on; when the
//     ring holds a wavefront's worth of local-estimate (shadow) rays the wave changes to RAY MODE: all lanes turn
//     (event, direction) pairs into ready rays (a ray whose roulette is already lost is dropped there), lanes take a
//     ready ray as soon as theirs has ended -- shadow rays run with nearly full wavefronts, independent of the photons
//     that caused them; with ONE radiance direction (an event is one ray, and the roulette ends most rays where they are made) there
//     is no ring: the event phase makes its event's ray ready itself and only survivors go to LDS, into a ready store of two
//     wavefronts (template parameter DIRECT);
//   * the batches of a driver's loop share ONE grid (PhiloxBatchStream: a lane carries its photon's batch in its Philox key, a
//     local-estimate ray in its info word; per-batch tally blocks in global memory), so that one batch's tail -- the few photons
//     with a thousand scatterings -- is filled by the next batch's photons;
//   * cell edges (and, when they fit, the extinction grid) are staged in LDS with coalesced loads; a field whose columns
//     each hold one run of one value (the I3RC Landsat scene) is read as one 8-byte record per column; other grids beyond an
//     XCD's L2 are read from a copy in 32-cell bricks; flux and radiance tallies are privatised per workgroup in LDS
//     (ds_add_f64) and flushed once with float64 atomics; large domains tally straight to HBM with float64 atomics;
//   * per-photon Philox4x32-10 streams keyed by (seed, batch) make a photon's path independent of the launch
//     geometry, of every scheduling threshold and of the number of GPUs;
//   * work counters live in scalar registers (advanced by s_bcnt1 of ballots in uniform control flow).
#pragma once
#include <cstddef>
#include "tally_block.hpp"
#include "event_flags.hpp"
#include "pass_decision.hpp"
#include "first_flight.hpp"
#include "tracer.hpp"
#include "tuning.hpp"

namespace i3rc {

enum LaneState { ST_TRACE = 0, ST_EVENT = 1, ST_DROPPED = 2, ST_NEW = 3, ST_DONE = 4,
                 ST_EXIT = 5 };   // an event known to end the photon (left through the top / onto a black surface): see the turnover quorum

// Work counters (I3RC_CNT_*) are kept per WAVE, in scalar registers: they are only ever advanced in uniform control
// flow by the population count of a ballot, so they cost no vector registers and no vector instructions.  The
// nested local-estimate path (replay / max cross-section builds) counts its tracer work per lane.
struct WaveCounters {   // 32 bits are enough: a wave hands its counts over every time it refills its photon reservoir
  uint32_t photons = 0, dropped = 0, steps = 0, scat = 0, surf = 0, top = 0, roul = 0, shadow = 0, calls = 0;
};
struct NestedCounters { uint32_t shadow = 0, calls = 0; };
// Two 16-bit counts in one register: what a lane of a fused flux launch counts for its photon's batch (photon_kernel, LANE_COUNTS).
// One event adds at most one to each count; a lane hands its counts over before either could leave its 16 bits.
struct LanePairs {
  uint32_t word = 0u;
  __device__ __forceinline__ void add(bool low, bool high) { word += (low ? 1u : 0u) + (high ? 1u << 16 : 0u); }
  __device__ __forceinline__ uint32_t low() const { return word & 0xffffu; }
  __device__ __forceinline__ uint32_t high() const { return word >> 16; }
  static __device__ __forceinline__ bool about_to_overflow(LanePairs a, LanePairs b) { return ((a.word | b.word) & ((1u << 15) | (1u << 31))) != 0u; }
};

__device__ __forceinline__ unsigned count_lanes(bool p) { return (unsigned)__popcll(__ballot(p)); }
// number of lanes below this one whose bit is set in a wave-uniform mask
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ void add_global(double *p, float v) { unsafeAtomicAdd(p, (double)v); }
__device__ __forceinline__ void add_global(double *p, double v) { unsafeAtomicAdd(p, v); }

// Kernel arguments that are only needed now and then -- the reservoir refill, the counter hand-over, the epilogue --
// are read from the kernarg segment where they are used (scalar loads) instead of living in scalar registers through
// the whole photon loop: the flux kernel wanted 106 of the 102 there are, and every spilled one comes back as a
// v_readlane, i.e. a vector instruction, in the event phase.  (The empty asm keeps the loads from being hoisted.)
struct KernelArgs { DevProblem P; RunArgs A; };   // the kernarg segment of photon_kernel: (P, A, ...)
static_assert(offsetof(KernelArgs, A) == sizeof(DevProblem) && sizeof(DevProblem) % 8 == 0 && alignof(RunArgs) == 8,
              "the second kernel argument must follow the first without padding");
typedef const __attribute__((address_space(4))) KernelArgs *ColdArgs;
typedef __attribute__((address_space(4))) DevProblem ColdProblem;   // (as a template argument: Tally<ColdProblem>)
__device__ __forceinline__ ColdArgs cold_args() {
  ColdArgs k = (ColdArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}


// BATCHED (fused multi-batch launch): every lane tallies into the block of ITS photon's batch (blk, worked out once per event
// phase), straight in global memory -- the hot words of a small domain are spread over several replicas of the block instead
// of being gathered in LDS, whose partial sums would have to be kept per batch.
template <class PR, bool BATCHED = false>
struct Tally {
  const PR &P;
  const Lds &L;
  double *blk;   // BATCHED: the lane's tally block (else the launch's one buffer, P.tally)
  // (the tally buffer's base addresses stay in scalar registers: reading them from the kernarg segment at every
  // tally -- see cold_args -- was measured: -8 % where the tallies go to global memory, nothing gained elsewhere)
  __device__ __forceinline__ double *base() const { return BATCHED ? blk : P.tally; }
  __device__ __forceinline__ void down(int col, float w) const {
    if (!BATCHED && P.ldsTallies) lds_add(&L.tDown[col], w); else add_global(base() + P.oDown + col, w);
  }
  // intensityByComponent(ix, iy, d, comp) (:574-579, :662-667)
  __device__ __forceinline__ void radiance(int comp, int d, int col, float v) const {
    const int i = (comp * P.nDir + d) * (P.nx * P.ny) + col;
    if (!BATCHED && P.ldsIntensity) lds_add(&L.tInt[i], v); else add_global(base() + P.oInt + i, v);
  }
  // upward flux at the top (:513) or downward flux at the surface (:531): one atomic for either
  __device__ __forceinline__ void boundary(bool top, int col, float w) const {
    if (!BATCHED && P.ldsTallies) lds_add((top ? L.tUp : L.tDown) + col, w);
    else add_global(base() + (top ? P.oUp : P.oDown) + col, w);
  }
  // Absorption (:644-647: fluxAbsorbed(ix, iy) and volumeAbsorption(ix, iy, iz) take the same increment): ONE tally, the cell's.  The
  // column's sum is the sum of its cells' and is formed from them after the launch (absorbed_columns_kernel, i3rc_hip.hip): the same
  // float64 additions in another order.  Scattered float64 atomics execute at the memory side, some 2e10 a second for the whole chip
  // (profiles/r05_atomic_rate.txt): two per scattering made the I3RC cases' absorbing versions (omega = 0.99) two to three times slower
  // than the conservative ones on the Landsat fields -- and nineteen times on the step cloud, whose 512 cells every wave of the chip
  // added to; a domain of few cells gathers them per workgroup in LDS (ldsVolume).
  __device__ __forceinline__ void absorbed(int cell, float w) const {
    if (!BATCHED && P.ldsVolume) lds_add(&L.tVol[cell], w); else add_global(base() + P.oVol + cell, w);
  }
  __device__ __forceinline__ bool volume_in_lds() const { return !BATCHED && P.ldsVolume; }
  __device__ __forceinline__ void absorbed_sum(int cell, double sum) const { add_global(base() + P.oVol + cell, sum); }   // (a lane's run in one cell: photon_kernel)
};

// PATH MOMENTS OF THE LOCAL ESTIMATE (EXTRA_RADIANCE_PATHS, PhiloxRadiancePathStream): per radiance direction and column the sums of c L
// and c L^2 over the contributions c that the launch adds to that radiance word, all components together -- radiancePath1 |
// radiancePath2, [nDir][ny][nx] each, in the column where the ray leaves the top.  L is the photon's float64 path register at the event
// (the register of the path tallies above) plus the ray's own length, which needs no tracing: a local-estimate ray runs straight to the
// top, (zMax - z) / uz in float64 (the host refuses a direction with uz <= 0).  The products are formed in float64 and added with float64
// atomics in global memory; a contribution of 0 adds nothing.
__device__ __forceinline__ void radiance_path_add(double *block, int nDir, int ncol, int d, int col, float con, double length) {
  const double cl = (double)con * length;
  // (never outside the block, whatever the indices)
  double *const at = block + (size_t)min((unsigned)d, (unsigned)(nDir - 1)) * (size_t)ncol + min((unsigned)col, (unsigned)(ncol - 1));
  add_global(at, cl);
  add_global(at + (size_t)nDir * (size_t)ncol, cl * length);
}

// computeIntensityContribution :1419-1611 for one event; adds straight into intensityByComponent.
// (RPATHS: ... and the contribution's path moments into `pathBlock`, `pathLen` being the photon's path up to the event: radiance_path_add)
template <int GRID, bool RPATHS = false, class Rng, class PR>
__device__ __forceinline__ void intensity_contribution(const PR &P, const Lds &L, Rng &rng, NestedCounters &cnt,
                                                       float weight, float x, float y, float z, int ix, int iy, int iz,
                                                       float dx, float dy, float dz, int component, int order,
                                                       double pathLen = 0.0, double *pathBlock = nullptr) {
  const int zIndexMax = P.nz + 1;
  const size_t ncol = (size_t)P.nx * P.ny;
  for (int d = 0; d < P.nDir; ++d) {
    const float ux = L.dirCos[3 * d], uy = L.dirCos[3 * d + 1], uz = L.dirCos[3 * d + 2];
    float normPF;
    if (component < 1) {
      normPF = 1.0f / kPi;
    } else {
      float proj = 0.0f;
      proj += dx * ux; proj += dy * uy; proj += dz * uz;
      if (fabsf(proj) > 1.0f) proj = copysignf(1.0f, proj);
      const float ang = acosf(proj);
      const size_t ncell = ncol * P.nz;
      const int pfi = max(P.pfIndex[(size_t)(component - 1) * ncell + cell_index(P, ix, iy, iz)], 1);
      const CompTables ct = load_tables(P.comp[component - 1]);
      const int n = ct.nFwd;
      const float *tab = ((P.useHybrid && order <= P.numOrdersOrig) ? ct.fwdOrig : ct.fwd) + (size_t)(pfi - 1) * n;
      normPF = lookup_phase(tab, n, ang) / ((4.0f * kPi) * fabsf(uz));
    }
    Ray r;
    r.x = x; r.y = y; r.z = z; r.ix = ix; r.iy = iy; r.iz = iz; r.dx = ux; r.dy = uy; r.dz = uz;
    r.set_direction<true>(L);   // (the general kernels' step: see Ray::slow)
    // ONE loop over the voxel steps of all the legs of this direction, the legs told apart by `stage` as in the light
    // phase of photon_kernel (0: plain local estimate, 1: small contribution, 2 / 3: the two legs of a large one).
    // Two loops one after the other (first leg, second leg) are what the compiler mishandled: see GridPlace.
    int stage = 0;
    float tauFree = 0.0f;
    r.acc = 0.0f; r.target = 0.0f;
    if (P.useRRI) {
      tauFree = -logf(fmaxf(kTiny, rng.next()));
      if (kPi * normPF <= P.zetaMin) { stage = 1; r.target = tauFree; }
      else { stage = 2; r.target = -logf(P.zetaMin / fmaxf(kTiny, kPi * normPF)); }   // tauMax
    }
    cnt.calls++;
    float con = 0.0f;
    for (;;) {
      cnt.shadow++;
      if (trace_step_lazy<GRID, false, true>(P, L, r, stage != 0) == STEP_CONTINUE) continue;   // (lazy: only a second leg needs the arrival's position, see the service phase of photon_kernel)
      const float tauB = r.acc;
      const bool outTop = r.iz >= zIndexMax;
      if (stage == 0) con = tauB >= 0.0f ? (weight * normPF) * expf(-tauB) : 0.0f;
      else if (stage == 1) {
        const float r2 = rng.next();
        con = (r2 <= kPi * normPF / P.zetaMin && outTop) ? weight * P.zetaMin / kPi : 0.0f;
      } else if (stage == 2) {
        if (outTop && tauB >= 0.0f) con = (weight * normPF) * expf(-tauB);
        else if (tauB >= 0.0f && r.iz >= 1) {   // second leg, up to the free path (not from below the grid: see the light phase)
          finish_arrival(r);                     // (the first leg has arrived at tauMax inside the grid: nothing else gets here)
          r.acc = 0.0f; r.target = tauFree; stage = 3;
          cnt.calls++;
          continue;
        }
      } else con = outTop ? weight * P.zetaMin / kPi : 0.0f;
      break;
    }
    if (P.limitContrib && con > P.maxContrib) {
      add_global(P.tally + P.oExc + component * P.nDir + d, con - P.maxContrib);
      con = P.maxContrib;
    }
    const Tally<PR> tl{P, L, nullptr};
    tl.radiance(component, d, (r.iy - 1) * P.nx + (r.ix - 1), con);
    if constexpr (RPATHS) {
      if (con != 0.0f)
        radiance_path_add(pathBlock, P.nDir, P.nx * P.ny, d, (r.iy - 1) * P.nx + (r.ix - 1), con, pathLen + ((double)P.zMax - (double)z) / (double)uz);
    }
  }
}

// (the primary template: the production stream, and with it the tag types derived from it)
template <class Rng>
struct RngInit {
  static __device__ __forceinline__ void init(PhiloxStream &g, const RunArgs &A) { g.init(A.seed0, A.seed1); }
  template <class AR>
  static __device__ __forceinline__ void start(PhiloxStream &g, const AR &A, long long i) {
    g.start((uint64_t)(A.firstPhoton + i));
  }
};
template <>
struct RngInit<PhiloxBatchStream> {
  static __device__ __forceinline__ void init(PhiloxBatchStream &g, const RunArgs &A) { g.init(A.seed0, A.seed1); }
};
template <>
struct RngInit<ReplayStream> {
  static __device__ __forceinline__ void init(ReplayStream &g, const RunArgs &A) { g.init(A.randoms, A.nRandoms); }
  template <class AR>
  static __device__ __forceinline__ void start(ReplayStream &g, const AR &A, long long i) { g.start(A.drawStart[i]); }
};

// THE OPTIONAL DIAGNOSTIC TALLY (ExtraTally, tally_block.hpp): photon_kernel<tag, false, true, GRID> -- the general flux kernel, the
// production stream under a tag type whose kExtra names the kind -- also fills one more block behind the counters of the packed tally
// buffer.  Where that block begins, for every kind:
__device__ __forceinline__ double *extra_block(double *tallyBase, long long countersOffset) { return tallyBase + extra_block_offset(countersOffset); }

// LEVEL FLUXES (EXTRA_LEVELS, PhiloxLevelStream): upward and downward flux through every layer interface, per column (levelFluxUp / levelFluxDown [nz + 1][ny][nx],
// level k = zEdges[k]).  The kernel tallies them at EVENT time from what the lane holds when its photon arrives: the weight (constant along the
// straight segment just traced), the direction, the arrival position and the layer the segment began in (one more register).  The
// tracer is not touched.  A segment from layer a to layer b (the tracer's own 1-based indices; nz + 1: out through the top, 0: onto
// the surface) adds its weight to levelFluxUp[a ... b - 1] going up, to levelFluxDown[b ... a - 1] going down; a new photon is
// counted at the face of its start layer that lies behind it, a reflected one at level 0, both in the tracer's own column.  The
// block -- levelFluxUp, levelFluxDown (nz + 1) * nx * ny words behind it -- is added to with float64 atomics in global memory: no LDS
// carve-up changes.

// The crossings of one straight segment that arrived at (x, y, z) in column `colArr`, layer index `izTo`, from layer `izFrom` with
// weight w.  The crossing point of level k is extrapolated BACK from the arrival along the direction and wrapped periodically with one
// floor (a path may be many domain widths long); its column comes from find_xy.  That is float32 arithmetic on the segment's end, not
// the tracer's own cell at that face: a crossing within rounding of a column's edge may be counted in the neighbouring column (the
// level's total is exact either way).  The level the segment ENDS on -- the top for an exit, the surface for an arrival there -- takes
// the tracer's own column, so that levelFluxUp[nz] and levelFluxDown[0] are fluxUp and fluxDown column by column.
template <class PR>
__device__ __forceinline__ void tally_level_crossings(const PR &P, const Lds &L, double *levelUp, float x, float y, float z, float dx, float dy, float dz,
                                                      int izFrom, int izTo, int colArr, int ixArr, int iyArr, float w) {
  const int nz = P.nz, ncol = P.nx * P.ny;
  const bool up = dz > 0.0f;
  int lo = up ? izFrom : izTo, hi = up ? izTo - 1 : izFrom - 1;
  lo = lo < 0 ? 0 : lo; hi = hi > nz ? nz : hi;          // (never outside the block, whatever the indices)
  double *const base = levelUp + (up ? 0 : (size_t)(nz + 1) * ncol);
  const int endLevel = up ? nz : 0;                      // the level an exit / a surface arrival ends on
  const bool endsOnBoundary = up ? izTo > nz : izTo < 1;
  const float widthX = P.xMax - P.x0, widthY = P.yMax - P.y0;
  for (int k = lo; k <= hi; ++k) {
    int col = colArr;
    if (!(endsOnBoundary && k == endLevel)) {
      const float back = (z - L.zE[k]) / dz;             // (>= 0: the level lies behind the arrival)
      float cx = x - dx * back, cy = y - dy * back;
      cx = cx - floorf((cx - P.x0) / widthX) * widthX;
      cy = cy - floorf((cy - P.y0) / widthY) * widthY;
      cx = fminf(fmaxf(cx, P.x0), P.xMax); cy = fminf(fmaxf(cy, P.y0), P.yMax);   // (rounding at the walls; a NaN ends at x0: always a column of the grid)
      int ix = ixArr, iy = iyArr;
      find_xy<true>(P, L, cx, cy, ix, iy);
      ix = ix < 1 ? 1 : (ix > P.nx ? P.nx : ix); iy = iy < 1 ? 1 : (iy > P.ny ? P.ny : iy);
      col = (iy - 1) * P.nx + (ix - 1);
    }
    add_global(base + (size_t)k * ncol + col, w);
  }
}

// ACTINIC FLUX by photon track length (EXTRA_TRACKS, PhiloxTrackStream): for every cell the sum, over all pieces of photon paths inside it, of w * l -- w the weight the
// photon carries along the piece (before the event at its end), l the float32 length the tracer itself steps -- as one float64 word per
// cell [nz][ny][nx]; normalised_actinic_flux (tally_block.hpp) turns it into the cell's mean actinic flux in units of the incident
// flux.  The kernel tallies it in the VOXEL-STEP phase: every step that is no tracer error adds w * step to the cell the photon was in BEFORE the step (trace_step_lazy,
// LENGTH), whether it reaches a face, snaps an index, wraps or leaves the grid; the arriving step advances nothing there, its length
// is the part finish_arrival forms in the event phase, tallied in the cell the photon stands in with the weight before the
// scattering.
// Where the field itself lies in LDS (GRID_LDS) and the launch has ncell * 8 more bytes of it, a workgroup keeps partial sums there
// (ds_add_f64 per step, one global atomic per non-zero word at its end): a small domain's few hundred words take a tenth of the
// scattered atomic rate in global memory, and a photon makes some sixty steps into them.  The region is carved BEHIND what lds_plan
// returns as its end, 8-byte aligned, in this instantiation and its launch alone; the host says so in bit 1 of DevProblem::ldsGrid,
// which no kernel reads otherwise.  Elsewhere: float64 atomics in global memory.
constexpr int kLdsGridTrackSums = 2;   // DevProblem::ldsGrid, bit 1 (launches of photon_kernel<PhiloxTrackStream, ...> only)
// first word of the track sums in a launch's dynamic LDS, given the end of its lds_plan -- the host's allocation and the kernel's pointer both
__host__ __device__ inline int track_sums_word(int planEnd) { return (planEnd + 1) & ~1; }
typedef __attribute__((address_space(3))) double lds_f64;
// one piece of a path: weight * length (exact in float64) into the cell's word -- the workgroup's partial sum, or the block in global memory
__device__ __forceinline__ void track_add(lds_f64 *sums, double *block, int cell, int ncell, float weight, float length) {
  const double v = (double)weight * (double)length;
  const unsigned at = min((unsigned)cell, (unsigned)(ncell - 1));   // (never outside the block, whatever the indices)
  if (sums) (void)__hip_atomic_fetch_add(sums + at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ds_add_f64
  else add_global(block + at, v);
}

// PATH LENGTHS of reflected and transmitted light (EXTRA_PATHS, PhiloxPathStream): per column the sums of w L and w L^2 over the photons
// that fluxUp and fluxDown count there -- w the weight the flux tally adds at that place (a surface arrival's: before the reflection), L
// the photon's geometric path since its start -- as four float64 fields [ny][nx]: pathUp1 | pathUp2 | pathDown1 | pathDown2.  L is a
// float64 register of the lane, the sum of exactly the pieces the actinic flux tallies, each float32 piece converted and added: every
// voxel step that is no tracer error (trace_step_lazy, LENGTH) and the part finish_arrival forms for an arriving step.  It is 0 for a
// new photon and carries on through a surface reflection; a photon the tracer drops tallies nothing.  The products are formed in
// float64 and added with float64 atomics in global memory -- two per photon ending, two more per reflection: no LDS carve-up changes.
__device__ __forceinline__ void path_add(double *block, int ncol, bool up, int col, float weight, double length) {
  const double wl = (double)weight * length;
  double *const at = block + (up ? 0 : 2 * (size_t)ncol) + min((unsigned)col, (unsigned)(ncol - 1));   // (never outside the block, whatever the indices)
  add_global(at, wl);
  add_global(at + ncol, wl * length);
}

// THE PATH HISTOGRAM of the same light (EXTRA_PATH_BINS, PhiloxBinStream): the same float64 path register, and at the same two places
// -- instead of two sums per column -- the weight and weight x path into the bin of float(L) (path_bin, tally_block.hpp: a search of
// fixed trip count over the float32 edges), domain-wide: binUp | binPathUp | binDown | binPathDown, nBins + 1 float64 words each, the
// last the overflow bin.  nBins and the edges travel in the device buffer DevProblem::dirCos points to in such a launch (the launch
// has no radiance directions: nDir == 0, and nothing else reads the pointer): word 0 nBins, then the nBins + 1 edges (BinTable).
// Where the launch's LDS has room (bit 2 of DevProblem::ldsGrid, plan_launch) a workgroup keeps the 4 (nBins + 1) sums as float64
// partial sums behind lds_plan's end -- at track_sums_word, as the track sums -- with the edges behind them: two ds_add_f64 per tally
// and one global float64 atomic per non-zero word at the workgroup's end, at any place of the extinction field.  Elsewhere: two float64
// atomics in global memory, the edges read from device memory.
constexpr int kLdsGridBinSums = 4;   // DevProblem::ldsGrid, bit 2 (launches of photon_kernel<PhiloxBinStream, ...> only)
// the region's length in float words for nBins bins -- the host's allocation and the kernel's carve-up both
__host__ __device__ inline int bin_region_words(int nBins) { return 2 * 4 * (nBins + 1) + (nBins + 1); }
// (what a wave keeps of it in scalar registers: the table itself is read through the kernel argument where it is needed)
struct BinTable {
  int nBins = 0;
  lds_f64 *sums = nullptr;           // the workgroup's partial sums (nullptr: the block in global memory is added to), its copy of the edges behind them
  // (the host has checked 1 <= nBins <= kMaxPathBins; the clamp keeps a kernel that reads anything else inside its LDS region and block)
  __device__ __forceinline__ void load(const float *table) { nBins = min(max(__builtin_amdgcn_readfirstlane(__float_as_int(table[0])), 1), kMaxPathBins); }
  __device__ __forceinline__ lds_float *lds_edges() const { return (lds_float *)(sums + 4 * (nBins + 1)); }
};
__device__ __forceinline__ void bin_add(const BinTable &B, const float *table, double *block, bool up, float weight, double length) {
  const float x = (float)length;
  const int b = B.sums ? path_bin(B.lds_edges(), B.nBins, x) : path_bin(table + 1, B.nBins, x);
  const unsigned at = (unsigned)path_bin_field(up ? 0 : 2, B.nBins) + (unsigned)b;   // (path_bin clamps: never outside the block)
  const double wv = (double)weight, wl = wv * length;
  if (B.sums) {
    (void)__hip_atomic_fetch_add(B.sums + at, wv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // ds_add_f64
    (void)__hip_atomic_fetch_add(B.sums + at + (B.nBins + 1), wl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else {
    add_global(block + at, wv);
    add_global(block + at + (B.nBins + 1), wl);
  }
}

// Wave-private reservoir of photon indices: one returning atomic per `chunk` photons instead of one per respawn
// round (the returning atomic costs microseconds; every wave would pay it in ~97 % of its event phases).  The two
// bounds are wave-uniform and held in scalar registers (readfirstlane tells the compiler so).
struct Reservoir {
  long long next, end;   // (XCD-aware order: positions in the sorted list; end < 0: every tile has run dry)
  // (Shorter chunks towards the end of a launch -- what is left shared out over all waves, down to one photon per lane -- were
  // tried in round 3: nothing at 1e8 photons, -1 % at 1.25e7, -6 % at 1e6.  A launch ends with its longest photon histories,
  // not with the last chunks.)
  __device__ __forceinline__ void refill() {   // call in uniform control flow only
    const ColdArgs k = cold_args();
    unsigned long long *const counter = k->A.workCounter;
    const int chunk = k->A.chunk;
    const long long nPhotons = k->A.nPhotons;
    unsigned long long base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(counter, (unsigned long long)chunk);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)__shfl((unsigned)base, 0, 64));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)__shfl((unsigned)(base >> 32), 0, 64));
    const long long b = (long long)(((unsigned long long)hi << 32) | lo);
    next = b < nPhotons ? b : nPhotons;
    end = b + chunk < nPhotons ? b + chunk : nPhotons;
  }
  // Fused multi-batch launch: the work counter hands out chunk numbers; a chunk lies within one batch (RunArgs).  `batch` is
  // the batch of the photons in hand (wave-uniform); end < 0 once the launch's chunks have run out or the host has called
  // the launch off (a look-ahead that is not wanted any more ends within one chunk per wave).
  unsigned batch = 0u;
  __device__ __forceinline__ void refill_batched() {   // call in uniform control flow only
    const ColdArgs k = cold_args();
    unsigned long long *const counter = k->A.workCounter;
    const unsigned chunk = (unsigned)k->A.chunk, perBatch = k->A.chunksPerBatch;
    const unsigned long long total = (unsigned long long)k->A.nBatches * perBatch;
    const long long nPhotons = k->A.nPhotons;
    unsigned long long c = total;
    if ((threadIdx.x & 63) == 0 && __hip_atomic_load(k->A.abortFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0)
      c = atomicAdd(counter, 1ull);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)__shfl((unsigned)c, 0, 64));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)__shfl((unsigned)(c >> 32), 0, 64));
    c = ((unsigned long long)hi << 32) | lo;
    if (c >= total) { next = 0; end = -1; return; }
    const unsigned b = (unsigned)(c / perBatch), j = (unsigned)(c - (unsigned long long)b * perBatch);
    batch = b;
    next = (long long)j * chunk;
    end = next + chunk < nPhotons ? next + chunk : nPhotons;
  }
  // XCD-aware order: positions in RunArgs::slabIds instead of photon numbers.  A wave takes from the slab of its own XCD
  // (whose L2 then holds that eighth of the field) and goes round the other slabs when that one has run dry.  How many
  // slabs of its round have run dry the wave keeps in LDS (read and written at refills only: no register for it in
  // kernels that have none to spare).
  __device__ __forceinline__ void refill_slabs(int *tried) {   // call in uniform control flow only
    const ColdArgs k = cold_args();
    SlabMeta *const m = k->A.slabMeta;
    const unsigned chunk = (unsigned)k->A.chunk;
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    next = end = -1;   // (nothing left: avail = 0 and end < 0)
    int slabTry = __builtin_amdgcn_readfirstlane(*tried);
    for (; slabTry < 8; ++slabTry) {
      const int s = (int)((xcc + (unsigned)slabTry) & 7u);
      const unsigned cnt = m->count[s], off = m->offset[s];
      unsigned base = 0;
      if ((threadIdx.x & 63) == 0) base = atomicAdd(&m->take[s], chunk);
      base = __builtin_amdgcn_readfirstlane((unsigned)__shfl(base, 0, 64));
      if (base < cnt) {
        next = (long long)off + base;
        end = (long long)off + (base + chunk < cnt ? base + chunk : cnt);
        break;
      }
    }
    if ((threadIdx.x & 63) == 0) *tried = slabTry;
  }
};

// The two passes that sort a launch's photons by start slab: a photon's start position is the first two deviates of its own
// stream (block 0, words 0 and 1: photon_kernel, part C), so its slab -- one of eight tiles of the domain -- is known before it
// is traced.  Pass 1 counts per workgroup (each workgroup owns a contiguous range of the launch's photons), the scan turns
// the counts into every workgroup's first position in every slab's list, pass 2 writes the photon numbers there: no global
// atomics, the same list for the same launch every time.  Both passes recompute the photon's first Philox block (about 1 ms
// for 1e8 photons; a first version with one global counter per slab took 490 ms: 1.5 million waves on eight words).
constexpr int kSlabSortBlocks = 2048;
__device__ __forceinline__ int start_slab(uint32_t seed0, uint32_t seed1, unsigned long long photon, int tx, int ty) {
  // tx x ty = 8 tiles of the domain (the host picks the squarest tiling: the smaller a tile's perimeter, the fewer photons
  // leave it): measured on the 128 x 128 Landsat field 2 x 4 6.50e8, 4 x 2 6.40e8, 1 x 8 6.35e8 photons/s
  const Philox4 o = philox4x32_10((uint32_t)photon, (uint32_t)(photon >> 32), 0u, 0u, seed0, seed1);
  const int sx = (int)(u32_to_unit_float(o.v[0]) * (float)tx), sy = (int)(u32_to_unit_float(o.v[1]) * (float)ty);
  return (sy >= ty ? ty - 1 : sy) * tx + (sx >= tx ? tx - 1 : sx);
}
__global__ void __launch_bounds__(256) slab_count_kernel(uint32_t seed0, uint32_t seed1, long long firstPhoton, long long n, long long span,
                                                         int tx, int ty, unsigned *blockCounts) {
  __shared__ unsigned cnt[8];
  if (threadIdx.x < 8) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * span, hi = lo + span < n ? lo + span : n;
  unsigned mine[8] = {};   // (per wave: only lane 0's copy is used)
  for (long long base = lo; base < hi; base += 256) {   // uniform trip count within the block
    const long long i = base + threadIdx.x;
    const int s = i < hi ? start_slab(seed0, seed1, (unsigned long long)(firstPhoton + i), tx, ty) : -1;
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[k] += (unsigned)__popcll(__ballot(s == k));
  }
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 8; ++k) atomicAdd(&cnt[k], mine[k]);
  __syncthreads();
  if (threadIdx.x < 8) blockCounts[blockIdx.x * 8 + threadIdx.x] = cnt[threadIdx.x];
}
// one thread per slab: the slab's size, then (after all sizes are known) every workgroup's first position in its list
__global__ void slab_scan_kernel(int nBlocks, const unsigned *blockCounts, SlabMeta *m, unsigned *blockBase) {
  __shared__ unsigned total[8];
  const int s = (int)threadIdx.x;
  unsigned c = 0;
  for (int b = 0; b < nBlocks; ++b) c += blockCounts[b * 8 + s];
  total[s] = c;
  __syncthreads();
  unsigned off = 0;
  for (int k = 0; k < s; ++k) off += total[k];
  m->count[s] = c; m->offset[s] = off; m->take[s] = 0u; m->fill[s] = 0u;
  for (int b = 0; b < nBlocks; ++b) { blockBase[b * 8 + s] = off; off += blockCounts[b * 8 + s]; }
}
__global__ void __launch_bounds__(256) slab_fill_kernel(uint32_t seed0, uint32_t seed1, long long firstPhoton, long long n, long long span,
                                                        int tx, int ty, const unsigned *blockBase, uint32_t *ids) {
  __shared__ unsigned cursor[8];
  if (threadIdx.x < 8) cursor[threadIdx.x] = blockBase[blockIdx.x * 8 + threadIdx.x];
  __syncthreads();
  const long long lo = (long long)blockIdx.x * span, hi = lo + span < n ? lo + span : n;
  for (long long base = lo; base < hi; base += 256) {
    const long long i = base + threadIdx.x;
    const int s = i < hi ? start_slab(seed0, seed1, (unsigned long long)(firstPhoton + i), tx, ty) : -1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned long long mask = __ballot(s == k);
      if (mask == 0ull) continue;
      const int leader = __builtin_ctzll(mask);
      unsigned at = 0;
      if ((int)(threadIdx.x & 63) == leader) at = atomicAdd(&cursor[k], (unsigned)__popcll(mask));
      at = (unsigned)__shfl(at, leader, 64);
      if (s == k) ids[at + (unsigned)lanes_below(mask)] = (uint32_t)i;
    }
  }
}

// Waves per SIMD an instantiation of photon_kernel is compiled for (its __launch_bounds__; the knobs and their measurements: tuning.hpp)
template <class Rng, bool INTENSITY, bool GENERAL, int GRID, bool TBL, bool MULTI>
constexpr int planned_waves() {
  // (radiance kernels keep two rays per lane live -- the photon's and a shadow ray's: 4 waves per SIMD give them 128 vector registers)
  if (INTENSITY && GENERAL) return 3;
  if (INTENSITY) return MULTI ? I3RC_MULTI_WAVES : I3RC_RADIANCE_WAVES;
  if (GENERAL || GRID == GRID_BRICKS) return I3RC_MIN_WAVES;   // (the bricked kernels: at most five workgroups per CU anyway)
  if (Rng::kBatched && !TBL) return MULTI ? I3RC_FUSED_WAVES - 2 : I3RC_FUSED_WAVES;
  return I3RC_FLUX_WAVES;   // (the specialised flux kernels; the fused table-in-LDS ones: 1024 threads, two workgroups per CU)
}
// What a wave of a STORE kernel (below) needs only when it fills its start store, or where a lane takes a photon from it -- the start
// layer, the reservoir's end, the count of its refills -- as four words of static LDS of the wave's own, instead of scalar registers
// that the whole photon loop would carry (eight waves per SIMD leave each 96 of them, and the kernels want more: tests/test_build_isa.py).
// (kRefills, where the kernel lands first flights -- FLIGHT --: the refills modulo four in the low two bits, above them the landed steps
// since the wave's last hand-over of its counters)
struct WaveStartState {
  enum Word { kLayer = 0, kEndLo = 1, kEndHi = 2, kRefills = 3, kWords = 4 };
  int *w = nullptr;
  __device__ __forceinline__ void save_end(long long end) const { w[kEndLo] = (int)(unsigned)end; w[kEndHi] = (int)(end >> 32); }
  __device__ __forceinline__ long long end() const {   // (wave-uniform: every lane reads the same words)
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane(w[kEndLo]), hi = (unsigned)__builtin_amdgcn_readfirstlane(w[kEndHi]);
    return (long long)(((unsigned long long)hi << 32) | lo);
  }
};
// Which instantiations start their photons a wavefront at a time from a per-wave START STORE in LDS (photon_kernel, part B of the event
// phase; StartSlot, tracer.hpp): the specialised flux kernels of plain launches wherever photon numbers are handed out in order -- the
// bricked kernels take theirs from the slab-sorted list and keep the start in the event phase, as every other kernel does.  A constant
// of the instantiation, derived from its template arguments: the host sizes the launch's LDS by the same function.
template <class Rng>
constexpr bool has_start_store(bool intensity, bool general, int grid, bool multi) {
  return !Rng::kReplay && !Rng::kBatched && Rng::kExtra == EXTRA_NONE && !intensity && !general && !multi && grid != GRID_BRICKS;
}
// GENERAL = false is the specialisation for the common problem class -- regular grid, ray tracing, one component,
// Lambertian albedo (no BRDF grid), Directional source, production RNG: the rare paths (grid searches, periodic
// re-wrapping loops, max-cross-section moves, BRDF lookups, component selection) are compiled out, which shrinks the
// loop's code and its scalar-register pressure.  GENERAL = true keeps every path behind run-time switches.
// TBL (round 3, specialised flux kernels): workgroups of 1024 threads, two per compute unit, that also keep the 40 KB of the
// inverse table's cosines (one entry) in LDS: the two dependent table reads of a scattering then come from LDS instead of
// L2 or beyond (+1.6 % on the step cloud, +22 % on Landsat-36; the launch chooses it: i3rc_hip.hip).
// DIRECT (round 4, radiance kernels, ONE radiance direction): no event ring.  With one direction an event is one ray, and with the
// roulette most rays end where they are made: the event phase itself turns its event into a ready ray (the EXPAND arithmetic, at
// the event phase's lane count -- what EXPAND had with a ring that an event phase half fills), only the survivors go to LDS, and
// the LDS the ring took pays for a ready store of two wavefronts: rays are traced when a wavefront of SURVIVORS has gathered.
// MULTI (round 5; with GENERAL = false, radiance kernels): the common class WIDENED by what production domains bring -- several components,
// an irregular x / y grid (only a photon's start looks its cell up: the tracer reads edges, whatever their spacing), a gridded surface
// (only a reflection looks its reflectance up) -- while max cross-section, the other photon sources and the replay stream stay with the
// general kernels.  For domains of SEVERAL components -- cloud + aerosol + gas is what
// Tools/PhysicalPropertiesToDomain.f95 makes --: the component of a scattering by a compare chain over the cell's cumulative
// extinctions (:637-638: the findIndex of (/0, cumulativeExt/), largest i with table(i) <= deviate), single-scattering albedo and
// phase-function entry read per cell and component (:642, :684-686), tables per component.  Everything else -- regular grid, ray
// tracing, no BRDF grid, Directional source -- as compiled out as in the one-component kernels; the deviates are drawn as the general
// kernels draw them (the component's from the stream's cursor), so that a MULTI launch traces the general kernels' photons.
template <class Rng, bool INTENSITY, bool GENERAL, int GRID, bool TBL = false, bool DIRECT = false, bool MULTI = false>
__global__ void __launch_bounds__(TBL ? 1024 : 256, (planned_waves<Rng, INTENSITY, GENERAL, GRID, TBL, MULTI>()))
photon_kernel(const DevProblem P, const RunArgs A, const int evThreshold, const int lightThreshold) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Lds L;
  constexpr bool STORE = has_start_store<Rng>(INTENSITY, GENERAL, GRID, MULTI);   // photons start a wavefront at a time: part B of the event phase
  constexpr bool FLAGS = STORE && I3RC_EVENT_FLAGS != 0;   // the event phase reads launch facts from DevProblem::eventFlags (event_flags.hpp)
  // ... and how their photon step spells its addresses and its outcome (StepForm, tracer.hpp): one switch of tuning.hpp per bit
  constexpr int STEP_FORM = !STORE ? 0 : (I3RC_STEP_BIASED_ADDRESS ? STEP_BIASED : 0) | (I3RC_STEP_STATE_SELECTS ? STEP_MASKS : 0) |
                                         (I3RC_STEP_COLD_ERROR ? STEP_COLD_ERROR : 0) | (I3RC_STEP_ADVANCE_MASKS ? STEP_ADVANCE_MASKS : 0);
  // ... and (round 17) "this launch can play roulette" as one bit of that word (kPlaysRoulette), made on the host
  constexpr bool ROULETTE_BIT = FLAGS && I3RC_ROULETTE_FLAG != 0;
  // ... and (round 18) land a zenith sun's photons at their first event where the wave makes their starts (first_flight.hpp; the bit
  // kFirstFlight of that word says that the launch does, and DevProblem::dirCos -- a flux launch has no directions -- then carries the table)
  constexpr bool FLIGHT = STORE && I3RC_FIRST_FLIGHT_TABLE != 0;
  // ... and how the head of their loop decides a pass and hands the decision to the event phase: one switch of tuning.hpp each
  constexpr bool PASS_BITS = STORE && I3RC_PASS_DECISION != 0;   // stop / runEvent / doTurn as bits of one 32-bit scalar (pass_decision.hpp)
  constexpr bool TURN_WORD = STORE && I3RC_TURN_ALL_WORD != 0;   // doTurn as a 64-bit -1 / 0 word made once per event phase
  // ... and their lanes' states in a numbering of their own, in which the three turnover states are the range's end -- NEW 3, DROPPED 4,
  // EXIT 5, the finished lane's DONE in DROPPED's place at 2 -- and `wantTurn` is one compare.  Every other kernel keeps LaneState's numbers.
  constexpr bool TURN_RANGE = STORE && I3RC_TURN_STATE_RANGE != 0;
  constexpr int kStDropped = TURN_RANGE ? (int)ST_DONE : (int)ST_DROPPED, kStDone = TURN_RANGE ? (int)ST_DROPPED : (int)ST_DONE;
  static_assert(!TURN_RANGE || (ST_NEW == 3 && kStDropped == 4 && ST_EXIT == 5 && kStDone < ST_NEW && ST_TRACE < ST_NEW && ST_EVENT < ST_NEW),
                "the turnover states are the states from ST_NEW on");
  // Which voxel step (trace_step_lazy): the general kernels' guarded division in a branch of its own, and -- CHAIN -- in the fused ring
  // kernels of a bricked field the specialised step as it was before zero cosines fell out of its minimum: with the minimum these two
  // instantiations ran out of scalar registers by two and kept the wave-uniform `adaptEvent` as a lane mask in a vector register,
  // the form tests/test_build_isa.py keeps out of the kernels (GridPlace).  Both want a zero cosine marked in Ray::slow.
  constexpr bool CHAIN = !GENERAL && Rng::kBatched && INTENSITY && !DIRECT && GRID == GRID_BRICKS;
  constexpr bool ZERO_IS_SLOW = GENERAL || CHAIN;
  lds_float *startSlots = nullptr;   // STORE: this wave's start store (StartSlot, tracer.hpp)
  constexpr bool TRACK = Rng::kExtra == EXTRA_TRACKS;   // actinic flux by track length (PhiloxTrackStream): tallied by the general flux kernel only
  lds_f64 *trackSums = nullptr;      // TRACK: the workgroup's partial sums of the block (nullptr: the block in global memory is added to)
  constexpr bool BINS = Rng::kExtra == EXTRA_PATH_BINS;   // the path histogram (PhiloxBinStream): tallied by the general flux kernel only
  BinTable bins;                     // BINS: the bins, and where this workgroup adds to them (bin_add)
  {
    // (one carve-up for the kernel and for the host's allocation: lds_plan, tracer.hpp)
    const LdsPlan lp = lds_plan(P, INTENSITY && !Rng::kReplay, DIRECT, GRID, INTENSITY, TBL ? 16 : 4, 0, STORE);
    lds_float *const base = (lds_float *)smem;
    if constexpr (STORE) startSlots = base + lp.startStore + (threadIdx.x >> 6) * (kStartWords * kStartSlots);
    const int ncol = P.nx * P.ny;
    L.xE = base + lp.xE; L.yE = base + lp.yE; L.zE = base + lp.zE;
    L.tUp = (lds_tally *)(base + lp.tallies); L.tDown = L.tUp + ncol; L.tVol = (lds_tally *)(base + lp.tVol);
    L.dirCos = base + lp.dirCos; L.dirTab = base + lp.dirTab; L.queue = base + lp.queue;
    L.tInt = (lds_tally *)(base + lp.tInt); L.ext = base + lp.ext; L.cosTab = base + lp.cosTab;
    if constexpr (TRACK && GRID == GRID_LDS)
      if (P.ldsGrid & kLdsGridTrackSums) trackSums = (lds_f64 *)(base + track_sums_word(lp.end));
    if constexpr (BINS) {
      bins.load(P.dirCos);
      if (P.ldsGrid & kLdsGridBinSums) bins.sums = (lds_f64 *)(base + track_sums_word(lp.end));
    }
  }
  if constexpr (BINS)
    if (bins.sums != nullptr) {
      for (int i = threadIdx.x; i < 4 * (bins.nBins + 1); i += blockDim.x) bins.sums[i] = 0.0;
      for (int i = threadIdx.x; i <= bins.nBins; i += blockDim.x) bins.lds_edges()[i] = P.dirCos[1 + i];
    }
  if constexpr (TRACK)
    if (trackSums != nullptr)
      for (int i = threadIdx.x; i < P.nx * P.ny * P.nz; i += blockDim.x) trackSums[i] = 0.0;
  for (int i = threadIdx.x; i < 3 * P.nDir; i += blockDim.x) L.dirCos[i] = P.dirCos[i];
  // coalesced staging of the edge vectors (and the extinction grid when it fits)
  for (int i = threadIdx.x; i <= P.nx; i += blockDim.x) L.xE[i] = P.xE[i];
  for (int i = threadIdx.x; i <= P.ny; i += blockDim.x) L.yE[i] = P.yE[i];
  for (int i = threadIdx.x; i <= P.nz; i += blockDim.x) L.zE[i] = P.zE[i];
  if (P.ldsTallies)
    for (int i = threadIdx.x; i < 2 * P.nx * P.ny; i += blockDim.x) L.tUp[i] = (tally_t)0;
  if (P.ldsVolume)
    for (int i = threadIdx.x; i < P.nx * P.ny * P.nz; i += blockDim.x) L.tVol[i] = (tally_t)0;
  if (GRID == GRID_LDS) {
    const int ncell = P.nx * P.ny * P.nz;
    for (int i = threadIdx.x; i < ncell; i += blockDim.x) L.ext[i] = P.totalExt[i];
  }
  if (GRID == GRID_COLBASE)                 // the base profile of column records over a per-layer value (DevProblem::colBase)
    for (int i = threadIdx.x; i < P.nz; i += blockDim.x) L.ext[i] = P.colBase[i];
  if (GRID == GRID_BRICKS && !INTENSITY) {   // the clear-air map of a bricked field (DevProblem::clearMap): flux kernels, see cell_extinction
    const int nWords = P.clearNx * (((P.ny - 1) >> P.clearShift) + 1);
    for (int i = threadIdx.x; i < nWords; i += blockDim.x) L.ext[i] = __uint_as_float(P.clearMap[i]);
  }
  if (P.ldsIntensity)
    for (int i = threadIdx.x; i < (P.ncomp + 1) * P.nDir * P.nx * P.ny; i += blockDim.x) L.tInt[i] = (tally_t)0;
  if (TBL) {
    const float *src = P.comp0.invCos + (size_t)(P.uniformPf >= 1 ? P.uniformPf - 1 : 0) * P.comp0.nInv;   // (else the table has one entry)
    for (int i = threadIdx.x; i < P.comp0.nInv; i += blockDim.x) L.cosTab[i] = src[i];
  }
  __syncthreads();
  if (INTENSITY && !Rng::kReplay) {   // what a ray of each radiance direction derives from it, once per workgroup (Ray::load_direction)
    for (int d = threadIdx.x; d < P.nDir; d += blockDim.x) {
      Ray t;
      t.dx = L.dirCos[3 * d]; t.dy = L.dirCos[3 * d + 1]; t.dz = L.dirCos[3 * d + 2];
      t.set_direction<ZERO_IS_SLOW>(L);
      t.store_direction(L.dirTab + 16 * d);
    }
    __syncthreads();
  }

  constexpr bool REPLAY = Rng::kReplay;        // per-photon fates are recorded by i3rc_hip_run_replay only
  constexpr bool BATCHED = Rng::kBatched;      // fused multi-batch launch: every lane knows its photon's batch (rng.batch)
  static_assert(!BATCHED || !GENERAL, "fused multi-batch launches: specialised kernels");
  constexpr bool LEVELS = Rng::kExtra == EXTRA_LEVELS;   // level fluxes (PhiloxLevelStream): tallied by the general flux kernel only
  static_assert(!LEVELS || (GENERAL && !INTENSITY && !TBL && !DIRECT && !MULTI), "level fluxes: the general flux kernel");
  static_assert(!TRACK || (GENERAL && !INTENSITY && !TBL && !DIRECT && !MULTI && !STORE && !BATCHED && !REPLAY && !LEVELS),
                "track lengths: the general flux kernel, no start store, not batched");
  // path-length moments (PhiloxPathStream) and the path histogram (PhiloxBinStream): the lane keeps its photon's path; tallied by the general flux kernel only
  constexpr bool PATH = Rng::kExtra == EXTRA_PATHS || BINS;
  static_assert(!PATH || (GENERAL && !INTENSITY && !TBL && !DIRECT && !MULTI && !STORE && !BATCHED && !REPLAY),
                "path lengths: the general flux kernel, no start store, not batched");
  // path moments of the local estimate (PhiloxRadiancePathStream): the lane keeps its photon's path as above, and the local estimate runs in
  // the nested order, which takes it (intensity_contribution, RPATHS); tallied by the general radiance kernel only, no ray queue
  constexpr bool RPATH = Rng::kExtra == EXTRA_RADIANCE_PATHS;
  static_assert(!RPATH || (GENERAL && INTENSITY && !TBL && !DIRECT && !MULTI && !STORE && !BATCHED && !REPLAY),
                "radiance path lengths: the general radiance kernel, not batched");
  constexpr bool PATH_REG = PATH || RPATH;   // the lane carries the float64 path register
  static_assert(!MULTI || (!GENERAL && !TBL && !Rng::kReplay && (INTENSITY || BATCHED)), "MULTI: the widened class -- radiance kernels, and the fused flux kernels (plain flux launches of the class run the general flux kernel)");
  // Work counters of a fused launch.  Flux kernels: exact per batch, gathered per lane (below).  Radiance kernels have no
  // vector register to spare for that: their counters stay per WAVE and are handed to the batch whose photons the wave was
  // given last -- photons and dropped photons (what the normalisation needs) are exact per batch, the others over the group.
#ifdef I3RC_FUSED_WAVE_COUNTS   /* (measurement knob: the fused flux kernels count per wavefront as the radiance kernels do) */
  constexpr bool LANE_COUNTS = false;
#else
  constexpr bool LANE_COUNTS = BATCHED && !INTENSITY;
#endif
  constexpr bool NEED_PID = REPLAY || GENERAL; // explicit photon sources are indexed by photon number
  const size_t ncell = (size_t)P.nx * P.ny * P.nz;
  const bool rayTracing = GENERAL ? (P.useRayTracing != 0) : true;
  const bool useBDRF = (GENERAL || MULTI) ? (P.useBDRF != 0) : false;
  const bool multiComp = (GENERAL || MULTI) ? (P.ncomp > 1) : false;   // (one component: no deviate is drawn for the choice, :637 -- the widened class too)
  const bool directional = GENERAL ? (A.srcKind == 0) : true;
  // Directional photons all start at z = z0 + (1 - spacing(1)) (zMax - z0): their start layer is wave-uniform
  const float zStart = P.z0 + (1.0f - spacingf(1.0f)) * (P.zMax - P.z0);
  int izStart = 1;
  find_z<true>(P, L, zStart, izStart);   // (once per wave: the specialised kernels take irregular layers too)
  const float rcpDeltaX = refined_rcp(P.deltaX), rcpDeltaY = refined_rcp(P.deltaY);
  const float surfaceZ = P.z0 + spacingf(P.z0);
  const bool blackSurface = !Rng::kReplay && !useBDRF && !(P.albedo > kTiny) && !INTENSITY;   // arrival at the surface ends the photon

  // RCP_ONCE (the specialised flux kernels of plain launches): the reciprocal of the inverse table's length, which every scattering
  // made again -- a conversion, v_rcp_f32 and its refinement on a value the launch fixes --, once per wave, in a scalar register
  constexpr bool RCP_ONCE = STORE && I3RC_TABLE_RCP_ONCE != 0;
  float tableRcp = 0.0f;
  if constexpr (RCP_ONCE) tableRcp = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(refined_rcp((float)P.comp0.nInv))));

  WaveCounters wc;
  NestedCounters nested;
  Rng rng;
  RngInit<Rng>::init(rng, A);
  Ray r;
  r.x = r.y = r.z = 0.0f; r.dx = r.dy = 0.0f; r.dz = -1.0f; r.ix = r.iy = r.iz = 1; r.acc = 0.0f; r.target = 0.0f;
  r.rx = r.ry = r.rz = 0.0f; r.slow = ZERO_IS_SLOW ? 1 : 0;   // (dx = dy = 0: see Ray::slow)
  r.ex = r.ey = r.ez = 0; r.cx = r.cy = r.cz = 1; r.nudge = 2.0f;
  float w = 0.0f;
  int order = 0;
  int st = ST_NEW;
  int izFrom = 1;                     // LEVELS: the layer the photon's current segment began in
  double pathLen = 0.0;               // PATH_REG: the photon's geometric path since its start (path_add, radiance_path_add)
  // Absorption where the tally goes to global memory: what a photon's CONSECUTIVE scatterings in one cell add to it leaves as one
  // atomic -- when the next scattering lies in another cell, or the photon ends (so that a fused launch's lane never holds a sum of
  // another batch's block).  In clouds whose cells are optically thick (an LES field: 55 m cells, free paths of 10 m) a photon is
  // scattered several times in a row in the cell it is in; the memory side takes some 2e10 scattered atomics a second, which one per
  // scattering reaches at 1.1e9 photons/s (Tally::absorbed).  The sum is float64: the same additions in another grouping.
  // (flux kernels: the radiance kernels, the general ones at three waves per SIMD and the fused table-in-LDS kernels at eight have no
  // three registers to spare -- with them they spilled 6 ... 20 bytes a lane)
  constexpr bool MERGE = I3RC_MERGE_ABSORPTION != 0 && !INTENSITY && !(Rng::kBatched && TBL);
  int pendCell = -1;
  double pendSum = 0.0;
  long long pid = -1;                 // photon number within the launch (NEED_PID builds)
  int fate = -1, fateCol = -1;        // REPLAY builds
  float fateW = 0.0f;
  // XCD-aware photon order: kernels on fields beyond an XCD's L2 (bricks), when the host has sorted the launch's photons
  constexpr bool SLABS = GRID == GRID_BRICKS && !Rng::kReplay;
  __shared__ int slabsTried[16];           // per wave (see Reservoir::refill_slabs; 16 waves in the 1024-thread instantiations)
  Reservoir res;
  int startAvail = 0;                      // STORE: photons made and not yet handed out, the ones in front of res.next (wave-uniform)
  if constexpr (BATCHED) res.refill_batched();
  else if (SLABS && A.slabIds != nullptr) {
    if ((threadIdx.x & 63) == 0) slabsTried[threadIdx.x >> 6] = 0;
    res.refill_slabs(&slabsTried[threadIdx.x >> 6]);
  } else res.refill();
  // STORE: what a wave needs only when it fills its start store, or where a lane takes a photon from it, lives in a few LDS words of
  // the wave's own (WaveStartState); the words exist in the STORE instantiations alone.
  WaveStartState startState;
  if constexpr (STORE) {
    __shared__ int startWords[16][WaveStartState::kWords];   // per wave (16 waves in the 1024-thread instantiations)
    static_assert(sizeof(startWords) <= kStaticLdsBytes && sizeof(slabsTried) <= kStaticLdsBytes && !SLABS,
                  "an instantiation's static LDS -- the start state or the slab round, never both -- is what the launch's LDS limit leaves room for");
    startState.w = startWords[threadIdx.x >> 6];
    startState.w[WaveStartState::kLayer] = izStart;
    startState.w[WaveStartState::kRefills] = 0;
    startState.save_end(res.end);
  }

  // ---- BATCHED: work counters per batch --------------------------------------------------------------------------------
  // The wave's scalar counters (wc) cannot tell the batches of its lanes apart: they only steer the thresholds here.  What
  // a batch's counter block is owed is gathered per LANE -- voxel steps in a register of their own, scatterings | roulette
  // plays and surface arrivals | exits through the top as two pairs of 16-bit counts, the deviates in the stream's own
  // count -- and handed over (a handful of atomics) when the lane's next photon belongs to another batch, when a count is
  // about to leave its 16 bits, and at the end.  Tracer calls need no count: every photon ends in exactly one of four ways
  // (top, surface, roulette, tracer error) and every event that does not end it starts a trace, so a batch's calls are its
  // scatterings + surface arrivals + exits through the top + dropped photons.  Photons are counted where they are handed
  // out (wave-uniform: resTaken), dropped ones at once (rare).
  uint32_t accSteps = 0u;                         // voxel steps
  LanePairs accA, accB;                           // scatterings (low) | roulette plays (high); surface arrivals | exits through the top
  uint32_t resTaken = 0u;                         // photons of the reservoir's batch handed out since the last hand-over
  const unsigned rep = BATCHED ? blockIdx.x % (unsigned)A.replicas : 0u;
  auto lane_block = [&](uint32_t b) -> double * {   // tally block of batch b for this workgroup (RunArgs)
    const ColdArgs k = cold_args();
    return k->P.tally + (size_t)(b * (unsigned)k->A.replicas + rep) * (size_t)(unsigned)k->A.blockStride;
  };
  auto counter_block = [&](uint32_t b) -> double * {   // ... and its counter block
    return cold_args()->A.counterBlocks + (size_t)(b * (unsigned)kCounterReplicas + (blockIdx.x & (unsigned)(kCounterReplicas - 1))) * I3RC_NUM_COUNTERS;
  };
  // (uniform control flow: the lanes with `want` hand their counts over.  The counts of all lanes that share a batch --
  // nearly always all of them -- are summed across the wave first and one lane adds them to the batch's counter block:
  // sixty-four lanes adding to the same seven words one after the other cost a launch 6 ms at its end and made chunks of
  // 256 photons half as fast as chunks of 1024.)
  auto flush_lanes = [&](bool want) {
    if constexpr (BATCHED) {
      unsigned long long todo = __ballot(want);
      while (todo != 0ull) {
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)rng.batch, (int)__builtin_ctzll(todo));
        const bool sel = want && rng.batch == b;
        // (one sum at a time, each ending in a scalar register: six at once cost the kernel six spilled vector registers)
        auto wave_total = [](uint32_t x) -> uint32_t {
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) x += (uint32_t)__shfl_xor((int)x, off, 64);
          return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
        };
        const uint32_t steps = wave_total(sel ? accSteps : 0u);
        const uint32_t scat = wave_total(sel ? accA.low() : 0u), roul = wave_total(sel ? accA.high() : 0u);
        const uint32_t surf = wave_total(sel ? accB.low() : 0u), top = wave_total(sel ? accB.high() : 0u);
        const uint32_t draws = wave_total(sel ? rng.take_used() : 0u);
        if ((threadIdx.x & 63) == 0) {
          double *const c = counter_block(b);
          if (steps) unsafeAtomicAdd(c + I3RC_CNT_CELL_STEPS, (double)steps);
          if (scat) unsafeAtomicAdd(c + I3RC_CNT_SCATTERINGS, (double)scat);
          if (roul) unsafeAtomicAdd(c + I3RC_CNT_ROULETTE, (double)roul);
          if (surf) unsafeAtomicAdd(c + I3RC_CNT_SURFACE_HITS, (double)surf);
          if (top) unsafeAtomicAdd(c + I3RC_CNT_EXITS_TOP, (double)top);
          if (scat + surf + top) unsafeAtomicAdd(c + I3RC_CNT_TRACER_CALLS, (double)(scat + surf + top));
          if (draws) unsafeAtomicAdd(c + I3RC_CNT_RNG_DRAWS, (double)draws);
        }
        if (sel) { accSteps = 0u; accA = accB = LanePairs(); }
        todo &= ~__ballot(sel);
      }
    }
  };
  auto hand_over_taken = [&](uint32_t b) {          // uniform control flow
    if (resTaken != 0u && (threadIdx.x & 63) == 0)
      unsafeAtomicAdd(counter_block(b) + I3RC_CNT_PHOTONS, (double)resTaken);
    resTaken = 0u;
  };

  // ---- Radiance (local estimate) through a per-wave RAY QUEUE -------------------------------------------------------
  // A scattering or reflection event does not trace its D local-estimate (shadow) rays itself and the photon does not
  // wait for them: the event is pushed as ONE record (position, cell, weight, incoming direction, table entry, and the
  // photon's Philox coordinates) into the wave's ring in LDS, and the photon goes on.  When the wave holds enough rays
  // to fill the wavefront (or the ring has no room for the next event phase, or the photons are finished) it changes to
  // RAY MODE, which has three phases:
  //   EXPAND   all 64 lanes turn one (event, direction) pair each into a ready-made ray -- phase-function factor (acos,
  //            table look-up), the ray's own Philox block, free path, roulette stage and target -- and put it into the
  //            wave's buffer of ready rays: the expensive part of a ray's start runs with full wavefronts;
  //   SERVICE  lanes whose ray has ended tally it and take the next ready ray (a dozen LDS reads), run when `liThr`
  //            lanes wait;
  //   STEP     one voxel step of every lane's ray -- nearly all lanes, since a lane whose ray ends is served soon.
  // Photons and shadow rays have their own registers (r, sr) and their own loops: the wave runs the photon loop until a
  // change of mode is due, then the ray loop, and back.
  // When nothing is left to hand out and fewer than kLowWater rays are still under way the wave goes back to its photons;
  // the unfinished rays go back to the ready buffer as they are and are resumed at the next change.  Every ray draws its two
  // deviates from a Philox block of its own, counter (photon, block of the event, direction + 1 in the fourth word; the
  // photon's own stream has 0 there): radiances do not depend on the schedule either.  Ray starts and ends use the
  // hardware log / exp / reciprocal (2 ulp): these are weights of a Monte Carlo estimate, not trajectories.
  // The replay build and max cross-section keep the reference's nested order (intensity_contribution).
  // (... and so does the radiance path tally: its contributions are made where the lane holds its photon's path)
  constexpr bool DEFER = INTENSITY && !Rng::kReplay && Rng::kExtra != EXTRA_RADIANCE_PATHS;
  // (max cross-section moves the photon inside the event: nested order there)
#ifdef I3RC_NESTED_BUILD
  // measurement build (tools/variant_bench.py build nested="-DI3RC_NESTED_BUILD"): the GENERAL kernels keep the reference's nested order
  // -- every ray traced where its event happens, the roulette played after the trace, libm in the weights -- with the production random
  // streams: a second implementation of :1419-1611 on the device to hold the ray queue against (profiles/r04_parity_xl.txt).  As a
  // run-time switch it cost the general radiance kernels nine spilled vector registers.
  const bool defer = DEFER && rayTracing && !GENERAL;
#else
  const bool defer = DEFER && rayTracing;
#endif
  enum { R_EMPTY = 0, R_TRACE = 1, R_ENDED = 2 };
  // (the schedule's levels and their measurements: tuning.hpp)
  constexpr int kTurnMin = Rng::kReplay ? 1 : (STORE ? I3RC_STORE_TURN_MIN : I3RC_TURN_MIN);
  constexpr int kTurnForce = Rng::kReplay ? 1 : (STORE ? I3RC_STORE_TURN_FORCE : I3RC_TURN_FORCE);
  constexpr int kExpandBatch = I3RC_EXPAND_BATCH;   // an expand phase runs when the ready buffer has room for this many rays
  constexpr int kDirectEnter = I3RC_DIRECT_ENTER, kDirectLeave = I3RC_DIRECT_LEAVE;   // DIRECT: the levels of ready / running rays at which a wave turns to its rays / back
  // (an event phase that would not fit -- possible when kDirectEnter is set above kDirectReady - 64 -- sends the wave to its rays first: wantSlots)
  static_assert(!DIRECT || (kDirectReady >= kDirectEnter && (kDirectReady & (kDirectReady - 1)) == 0), "the ready store holds the entry level; a power of two");
  constexpr int kLowWater = I3RC_LOW_WATER, kStepAhead = I3RC_STEP_AHEAD, kPhotonStepAhead = I3RC_PHOTON_STEP_AHEAD;
  bool wantSlots = false, photonsLeft = true;         // wave-uniform
  unsigned qTail = 0u, qHeadEv = 0u, qHeadSub = 0u;   // events pushed / events expanded completely / rays expanded of event qHeadEv
  unsigned rdHead = 0u, rdTail = 0u;                  // ready rays taken / made
  constexpr int kReady = DIRECT ? kDirectReady : kReadyRays;     // slots of the wave's ready store
  lds_float *const qBase = L.queue + (threadIdx.x >> 6) * (kRecWords * P.rayQueueCap + kReadyWords * kReady);
  lds_float *const rdBase = qBase + kRecWords * P.rayQueueCap;   // ready rays (ReadyRay, tracer.hpp)
  const unsigned qMask = (unsigned)P.rayQueueCap - 1u;
  const unsigned qMagic = ((1u << 20) + (unsigned)P.nDir - 1u) / (unsigned)(P.nDir > 0 ? P.nDir : 1);   // t / nDir = (t * qMagic) >> 20 for t < nDir + 64 <= 319 (nDir <= 255)
  bool pendingShadow = false;
  float wI = 0.0f, inDx = 0.0f, inDy = 0.0f, inDz = 0.0f;   // of the event being pushed
  int evInfo = 0;   // (an EventInfo word)

  // Thresholds: fixed when the caller asks for them (> 0), else adapted by every wave to its own photons at every
  // reservoir refill.  Event phase: the longer the photons' own traces (voxel steps per event), the more a
  // lane loses by waiting for others, so the threshold falls with the steps per event: 44 - 2 steps per event for the flux
  // kernels, 44 - 1.2 steps per event for the radiance kernels, within 12 ... 44 (adapt_thresholds; until round 4 58 / sqrt(steps per event)).  Ray mode's service phase: likewise with the length of
  // the shadow rays, 70 / sqrt(steps per ray) within 16..32.  Thresholds only schedule work: no photon path depends on them.
  int evThr = evThreshold > 0 ? evThreshold : -evThreshold;
  int liThr = lightThreshold > 0 ? lightThreshold : -lightThreshold;
  const bool adaptEvent = evThreshold < 0, adaptLight = DEFER && lightThreshold < 0;
  uint32_t raysStarted = 0;   // tracer calls for shadow rays since the last refill (wave-uniform)
  uint32_t raysSkipped = 0;   // local-estimate rays known to contribute nothing before any tracing (lost roulette): whole kernel, per wave
  uint32_t refills = 0;       // visits of the work counter by this wave
  // re-fit the thresholds to what this wave has seen since its last hand-over (uniform control flow only)
  uint32_t raysSeen = 0;      // shadow rays since the last hand-over
  auto adapt_thresholds = [&]() {
    if (adaptEvent) {
      const float events = (float)(wc.scat + wc.photons + wc.surf), steps = (float)wc.steps;
      if (events > 0.0f && steps > 0.0f) {
        const int t = (int)(44.0f - (INTENSITY ? I3RC_EVTHR_SLOPE_RADIANCE : I3RC_EVTHR_SLOPE_FLUX) * (steps * __builtin_amdgcn_rcpf(events)));
        evThr = __builtin_amdgcn_readfirstlane(t < 12 ? 12 : (t > 44 ? 44 : t));
      }
    }
    if (adaptLight) {
      raysSeen += raysStarted; raysStarted = 0u;
      if (raysSeen > 0u && wc.shadow > 0u) {
        const int t = (int)(I3RC_LITHR_COEF * __builtin_amdgcn_rsqf((float)wc.shadow * __builtin_amdgcn_rcpf((float)raysSeen)));
        liThr = __builtin_amdgcn_readfirstlane(t < I3RC_LITHR_MIN ? I3RC_LITHR_MIN : (t > 32 ? 32 : t));
      }
    }
  };
  // hands the wave's work counters over to the tally buffer (uniform control flow only)
  auto flush_counters = [&]() {
    adapt_thresholds();
    raysSeen = 0u;
    if constexpr (BATCHED && !LANE_COUNTS) {   // per wave, to the batch in hand (LANE_COUNTS above)
      uint32_t draws = rng.take_used();
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) draws += (uint32_t)__shfl_xor((int)draws, off, 64);
      if ((threadIdx.x & 63) == 0) {
        double *const c = counter_block(res.batch);
        const uint32_t v[8] = {wc.steps, wc.scat, wc.surf, wc.top, wc.roul, wc.shadow, wc.scat + wc.surf + wc.top + wc.calls, draws};
        const int at[8] = {I3RC_CNT_CELL_STEPS, I3RC_CNT_SCATTERINGS, I3RC_CNT_SURFACE_HITS, I3RC_CNT_EXITS_TOP, I3RC_CNT_ROULETTE,
                           I3RC_CNT_SHADOW_STEPS, I3RC_CNT_TRACER_CALLS, I3RC_CNT_RNG_DRAWS};
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (v[k] != 0u) unsafeAtomicAdd(c + at[k], (double)v[k]);
        if (raysSkipped != 0u) unsafeAtomicAdd(c + I3RC_CNT_RAYS_SKIPPED, (double)raysSkipped);
      }
      raysSkipped = 0u;
    }
    // FLIGHT: the steps of the first flights that the fill landed instead of stepping (WaveStartState::kRefills, its upper thirty bits)
    uint32_t landedSteps = 0u;
    if constexpr (FLIGHT) {
      const unsigned word = (unsigned)__builtin_amdgcn_readfirstlane(startState.w[WaveStartState::kRefills]);
      landedSteps = word >> 2;
      startState.w[WaveStartState::kRefills] = (int)(word & 3u);
    }
    if (!BATCHED && (threadIdx.x & 63) == 0) {   // (BATCHED flux kernels: per lane and batch, see flush_lanes)
      // (STORE: tracer calls are derived, not counted -- every trace ends in exactly one scattering, surface arrival, exit through the
      // top or tracer drop, each counted where the event phase serves it, and every trace has ended when the launch has: over a launch
      // the sum is the number of traces started, which is all the host ever sees of these hand-overs)
      const uint32_t calls = STORE ? wc.scat + wc.surf + wc.top + wc.dropped : wc.calls;
      const uint32_t c[9] = {wc.photons, wc.dropped, FLIGHT ? wc.steps + landedSteps : wc.steps, wc.scat, wc.surf, wc.top, wc.roul, wc.shadow, calls};
      const ColdArgs ka = cold_args();
      double *const counters = ka->P.tally + ka->P.oCnt;
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if (c[k] != 0u) unsafeAtomicAdd(counters + k, (double)c[k]);
    }
    wc = WaveCounters();
  };
  // One (event, direction) pair -> a ready-made local-estimate ray (:1473-1559): the phase-function factor (acos, table
  // look-up), the ray's own Philox block (counter: photon, block of its event, direction + 1), free path, roulette stage and
  // target.  false: the ray is known to contribute nothing and is not traced (below).  Called by the EXPAND phase of ray mode
  // (the event from the wave's ring) and, in DIRECT kernels, by the event phase itself (the event from registers).
  // (the event's and the ray's info words: EventInfo, RayInfo, tracer.hpp)
  auto make_ray = [&](const auto &Px, const auto &Ax, int info, float inX, float inY, float inZ, uint32_t photonLo, uint32_t photonHi,
                      uint32_t eventBlock, uint32_t batch, int dIdx, float &rayWord, float &normOut, float &tauFreeOut, float &targetOut) -> bool {
    const int comp = EventInfo::component(info);
    const float uz = L.dirCos[3 * dIdx + 2];
    float norm;
    if (comp < 1) norm = 1.0f / kPi;
    else {
      float proj = 0.0f;
      proj += inX * L.dirCos[3 * dIdx]; proj += inY * L.dirCos[3 * dIdx + 1]; proj += inZ * uz;
      if (fabsf(proj) > 1.0f) proj = copysignf(1.0f, proj);
#ifdef I3RC_FAST_ACOS
      const float ang = fast_acos(proj);
#else
      const float ang = acosf(proj);
#endif
      const int pfi = EventInfo::table_entry(info);
      const CompTables ct = (GENERAL || MULTI) ? load_tables(Px.comp[comp - 1]) : load_tables(Px.comp0);
      const float *tab = (EventInfo::hybrid(info) ? ct.fwdOrig : ct.fwd) + (size_t)(pfi - 1) * ct.nFwd;
      norm = fast_div(lookup_phase_fast(tab, ct.nFwd, ang), (4.0f * kPi) * fabsf(uz));
    }
    int stg = 0;
    bool won = false;
    float tauFree = 0.0f, target = 0.0f;
    if (Px.useRRI) {
      const Philox4 q4 = philox4x32_10(photonLo, photonHi, eventBlock, (uint32_t)dIdx + 1u, Ax.seed0, BATCHED ? Ax.seed1 + batch : Ax.seed1);
      rng.count_draws(2u);
      tauFree = -fast_log(fmaxf(kTiny, u32_to_unit_float(q4.v[0])));
      // small contribution: it counts -- with the weight of the roulette's bound -- with probability pi normPF / zetaMin
      // (:1551-1559); the deviate is compared here, the outcome travels in the ray's info word (RayInfo::won)
      const float r2 = u32_to_unit_float(q4.v[1]);
      if (kPi * norm <= Px.zetaMin) { stg = 1; won = r2 * Px.zetaMin <= kPi * norm; target = tauFree; }
      else { stg = 2; target = -fast_log(fast_div(Px.zetaMin, fmaxf(kTiny, kPi * norm))); }   // tauMax
    }
    rayWord = __int_as_float(RayInfo::pack(comp, dIdx, stg, won, batch));   // (as the ready ray's slot holds it)
    normOut = norm; tauFreeOut = tauFree; targetOut = target;
    // A small contribution that has lost its roulette (:1554: the deviate is independent of the path) is 0 whatever
    // the trace would find: such a ray is not traced at all -- the same estimator, evaluated lazily.  (The
    // reference traces first and draws afterwards; the replay build keeps that order.)
    return stg != 1 || won;   // (a small contribution that lost its roulette is dropped; stages 0 and 2 are always traced)
  };
  // a photon's record for i3rc_hip_run_replay; production builds keep no per-photon record
  auto close_photon = [&]() {
    if (REPLAY) {
      if (A.fate) {
        A.fate[pid] = fate; A.fateColumn[pid] = fateCol; A.fateWeight[pid] = fateW; A.fateOrder[pid] = order;
        A.drawsUsed[pid] = (int32_t)rng.draws_of_photon();
      }
    }
    rng.close();
  };
  // diagnostic build only (-DI3RC_PROFILE_PHASES, tools/phase_profile.py): where do a wave's cycles go?  Per phase kind:
  // cycles (s_memtime), number of phases, lanes served.  The results leave through the volume-absorption tally.
  enum { PH_EVENT = 0, PH_STEP = 1, PH_RAYSTEP = 2, PH_EXPAND = 3, PH_SERVICE = 4, PH_KINDS = 5 };
#ifdef I3RC_PROFILE_PHASES
  unsigned long long profCycles[PH_KINDS] = {}, profCount[PH_KINDS] = {}, profLanes[PH_KINDS] = {};
  unsigned long long profMark = 0;
  unsigned long long profWrap[4] = {};   // STORE: photon-step phases in which no lane / x only / y only / both axes crossed a side wall (index = axis bits)
  const unsigned long long profStart = __builtin_amdgcn_s_memtime();
#define PROF_BEGIN() (profMark = __builtin_amdgcn_s_memtime())
#define PROF_END(kind, lanes) do { profCycles[kind] += __builtin_amdgcn_s_memtime() - profMark; profCount[kind]++; profLanes[kind] += (unsigned long long)(lanes); } while (0)
#else
#define PROF_BEGIN() do {} while (0)
#define PROF_END(kind, lanes) do {} while (0)
#endif
  for (;;) {
    if (DEFER) {
      // ============================================================================================== RAY MODE?
      // enough local-estimate rays to fill the wavefront (or no room for the next event phase, or no photons left)?
      const int work = DIRECT ? (int)(rdTail - rdHead) : (int)((qTail - qHeadEv) * (unsigned)P.nDir - qHeadSub) + (int)(rdTail - rdHead);
      photonsLeft = __ballot(st != kStDone) != 0ull;
      if (work > 0 && (work >= (DIRECT ? kDirectEnter : 64) || !photonsLeft || wantSlots)) {
        wantSlots = false;
        // this lane's shadow ray: registers of the ray loop only (rays still under way when the wave leaves go back to the
        // ready buffer), so that the photon loop's register allocation knows nothing of them and the other way round
        Ray sr;                                             // (every field is set when a lane takes a ray, before any use: no initial
        int rst = R_EMPTY, sInfo;                           //  values, which would cost a register copy each at every pass of the photon loop)
        float sW, sNorm, sTauFree;                          // state; info word; weight, phase-function factor, free path
        // (One back edge only: EXPAND runs in a loop of its own and SERVICE goes on into the step phase.  With three ways
        // back to the loop's head -- after an expand, after a service, after the steps -- the compiler kept the rays' 27
        // registers in one set at the head and in another at the latch and copied them to and fro, some forty vector
        // moves in every pass: "Exchanging two register sets")
        for (;;) {
          if constexpr (!DIRECT) for (;;) {
            const int ringRays0 = (int)((qTail - qHeadEv) * (unsigned)P.nDir - qHeadSub);
            const int ready0 = (int)(rdTail - rdHead);
            if (!(ringRays0 > 0 && ready0 <= kReady - kExpandBatch)) break;
            // ------------------------------------------------------------ EXPAND phase: (event, direction) -> ready ray
            const int room = kReady - ready0;
            const int n = ringRays0 < room ? ringRays0 : room;
            const int lane = (int)(threadIdx.x & 63);
            PROF_BEGIN();
            const ColdArgs kx = cold_args();   // (the problem through the kernarg segment, as in the event phase)
            const auto &Px = kx->P;
            const auto &Ax = kx->A;
            bool keep = false;
            float evRayWord = 0.0f, evNorm = 0.0f, evTauFree = 0.0f, evTarget = 0.0f;
            lds_float *evRec = qBase;
            if (lane < n) {                                                  // next radiance direction (:1473-1510)
              const unsigned t = qHeadSub + (unsigned)lane;
              const unsigned eOff = (t * qMagic) >> 20;
              const int dIdx = (int)(t - eOff * (unsigned)Px.nDir);
              const EventRecord<BATCHED> ev{qBase + ((qHeadEv + eOff) & qMask), Px.rayQueueCap};
              const uint32_t photonHi = ev.photon_hi(), batch = ev.batch();   // (one word of the record: EventRecord)
              keep = make_ray(Px, Ax, ev.info(), ev.in_dx(), ev.in_dy(), ev.in_dz(), ev.photon_lo(), photonHi, ev.philox_block(), batch, dIdx,
                              evRayWord, evNorm, evTauFree, evTarget);
              evRec = ev.rec;
            }
            const unsigned long long keepMask = __ballot(keep);
            if (keep) {
              const EventRecord<BATCHED> ev{evRec, Px.rayQueueCap};
              ReadyRay::store_from(rdBase + ((rdTail + (unsigned)lanes_below(keepMask)) & (unsigned)(kReady - 1)), kReady, ev,
                                   __float_as_int(evRayWord), evNorm, evTauFree, evTarget);
            }
            {   // ring bookkeeping (wave-uniform)
              const unsigned t = qHeadSub + (unsigned)n;
              const unsigned e = (t * qMagic) >> 20;
              qHeadEv += e; qHeadSub = t - e * (unsigned)Px.nDir;
              const unsigned kept = (unsigned)__popcll(keepMask);
              rdTail += kept;
              raysSkipped += (unsigned)n - kept;
            }
            PROF_END(PH_EXPAND, n);
          }
          const int ringRays = DIRECT ? 0 : (int)((qTail - qHeadEv) * (unsigned)P.nDir - qHeadSub);   // rays waiting in the ring, not yet expanded
          const int ready = (int)(rdTail - rdHead);                                        // ready-made rays
          const unsigned long long actMask = __ballot(rst == R_TRACE), endMask = __ballot(rst == R_ENDED);
          const int nAct = (int)__popcll(actMask), nIdle = 64 - nAct;
          // with photons still to run, the wave leaves its rays once there is nothing left to hand out and few are under way
          // (no more rays can be made ready at this point: the ring is empty, or the ready buffer is full)
          // (DIRECT: see kDirectLeave -- nothing left to hand out and only a few rays still under way)
          const bool leaving = DIRECT ? (photonsLeft && ready == 0 && nAct < kDirectLeave)
                                      : (ringRays == 0 && photonsLeft && ready + nAct < kLowWater);   // too few for a wavefront: gather more first
          const bool canServe = endMask != 0ull || (!leaving && ready > 0 && nIdle > 0);
          const bool serve = canServe && (nIdle >= liThr || nAct == 0 || leaving);
          if (serve) {
            // ------------------------------------------------------------ SERVICE phase (shadow-ray ends and starts)
            PROF_BEGIN();
            const ColdArgs kx = cold_args();
            const auto &Px = kx->P;
            bool secondLeg = false;
            if (rst == R_ENDED) {                                           // the ray that just ended (:1517-1596)
              double *rayBlk = nullptr;                                     // (fused launches: the tally block of the ray's batch)
              if constexpr (BATCHED) rayBlk = lane_block(RayInfo::batch(sInfo));
              const Tally<ColdProblem, BATCHED> tally{Px, L, rayBlk};
              const float tauB = sr.acc;
              const bool outTop = sr.iz >= Px.nz + 1;
              const int comp = RayInfo::component(sInfo), dIdx = RayInfo::direction(sInfo), stage = RayInfo::stage(sInfo);
              const float direct = tauB >= 0.0f ? (sW * sNorm) * fast_exp(-tauB) : 0.0f;   // plain local estimate
              const float capped = outTop ? sW * Px.zetaMin * (1.0f / kPi) : 0.0f;          // roulette survivor
              float con = 0.0f;
              if (stage == 0) con = direct;
              else if (stage == 1) con = RayInfo::won(sInfo) ? capped : 0.0f;
              else if (stage == 2) {
                if (outTop) con = direct;
                else if (tauB >= 0.0f && sr.iz >= 1) {                      // second leg, up to the free path (:1576-1587)
                  // (the first leg has ARRIVED at tauMax inside the grid -- the only way to get here: an exit through the bottom has
                  // iz < 1, a failed trace tauB = -2 -- and its last advance is still to be made: trace_step_lazy.  Every other ray
                  // that ends at its target contributes nothing, wherever it stands: stages 1 and 3 count only through the top.)
                  finish_arrival(sr);
                  sr.acc = 0.0f; sr.target = sTauFree; sInfo = RayInfo::to_second_leg(sInfo); rst = R_TRACE; secondLeg = true;
                }
                // (a first leg that left through the BOTTOM -- a downward radiance direction -- gets no second leg: the
                // reference starts one from outside the grid, reads zPosition(0) / totalExt(:, :, 0) out of bounds and
                // discards the outcome, since only an exit through the top counts; the contribution is 0 either way)
              } else con = capped;
              if (rst == R_ENDED) {
                if (Px.limitContrib && con > Px.maxContrib) {                // :1598-1609
                  add_global(tally.base() + Px.oExc + comp * Px.nDir + dIdx, con - Px.maxContrib);
                  con = Px.maxContrib;
                }
                // (most rays of the roulette end without a contribution: no atomic for adding nothing -- on the radar
              // field the radiance atomics were 1.4 KB of HBM writes per photon and half of the waves' cycles were waits)
              if (con != 0.0f) tally.radiance(comp, dIdx, (sr.iy - 1) * Px.nx + (sr.ix - 1), con);
                rst = R_EMPTY;
              }
            }
            // hand ready rays to the free lanes, in order
            const unsigned long long freeMask = __ballot(rst == R_EMPTY);
            const int nFree = (int)__popcll(freeMask);
            const int take = leaving ? 0 : (nFree < ready ? nFree : ready);   // (a wave about to leave ends its rays but takes no new ones)
            const int rank = lanes_below(freeMask);
            if (rst == R_EMPTY && rank < take) {
              const ReadyRay::Words in = ReadyRay::load(rdBase + ((rdHead + (unsigned)rank) & (unsigned)(kReady - 1)), kReady);
              sr.x = in.x; sr.y = in.y; sr.z = in.z; sr.ix = in.ix; sr.iy = in.iy; sr.iz = in.iz;
              sInfo = in.info; sW = in.weight; sNorm = in.norm; sTauFree = in.freePath; sr.target = in.target; sr.acc = in.opticalPath;
#ifdef I3RC_NO_DIRTAB   /* (measurement knob: the direction's derived values worked out at every ray start, as before round 4) */
              const int dIdx = RayInfo::direction(sInfo);
              sr.dx = L.dirCos[3 * dIdx]; sr.dy = L.dirCos[3 * dIdx + 1]; sr.dz = L.dirCos[3 * dIdx + 2];
              sr.set_direction<ZERO_IS_SLOW>(L);
#else
              sr.load_direction(L.dirTab + 16 * RayInfo::direction(sInfo));
#endif
              rst = R_TRACE;
            }
            rdHead += (unsigned)take;
            const unsigned started = (unsigned)take + count_lanes(secondLeg);   // every start is one tracer call
            wc.calls += started;
            raysStarted += started;
            PROF_END(PH_SERVICE, __popcll(endMask) + take);
          }
          // rays still under way go back to the ready buffer as they are.  (A wave that leaves has taken no new rays in the
          // service phase just before, but rays that ended there may have begun their second leg: with those the rays under
          // way may no longer fit beside the ready ones -- then the wave stays, as it did when the next pass re-counted.)
          const unsigned long long backMask = __ballot(rst == R_TRACE);   // (after the service phase, if there was one)
          const int nBack = (int)__popcll(backMask);
          const int readyNow = (int)(rdTail - rdHead);
          if ((leaving && (DIRECT || ready + nBack < kLowWater)) || (nBack == 0 && readyNow == 0 && ringRays == 0)) {
            if (rst == R_TRACE) {
              ReadyRay::store(rdBase + ((rdTail + (unsigned)lanes_below(backMask)) & (unsigned)(kReady - 1)), kReady, sr.x, sr.y, sr.z, sr.ix, sr.iy, sr.iz,
                              sInfo, sW, sNorm, sTauFree, sr.target, sr.acc);
            }
            rdTail += (unsigned)nBack;
            wc.calls -= (unsigned)nBack;      // (they are counted again when they are taken up: one tracer call each, whatever the schedule)
            raysStarted -= (unsigned)nBack;
            break;
          }
          // -------------------------------------------------------------- VOXEL-STEP phase (shadow rays)
          // (a second step in the same pass while the next service phase is some lanes away: the phase logic above --
          // ballots, counts, the decisions -- is paid once for both; written out twice, see the photons' step phase)
          auto ray_step = [&]() {
            const bool tracing = rst == R_TRACE;
            const unsigned nTracing = count_lanes(tracing);
            wc.shadow += nTracing;
            PROF_BEGIN();
            if (tracing) {   // a failed shadow ray contributes nothing (:1531-1535: its optical path is -2)
              // (an arrival: see the service phase.  The ray's own stage says whether it has a target: the wave-uniform P.useRRI says the
              // same, and as a run-time flag in this loop it came out as a lane mask made under another loop's exec mask -- GridPlace's trap,
              // caught by tests/test_build_isa.py)
              if (trace_step_lazy<GRID, false, GENERAL, !DIRECT, false, CHAIN>(P, L, sr, RayInfo::stage(sInfo) != 0) != STEP_CONTINUE) rst = R_ENDED;   // (ring kernels: the short form, see trace_step_lazy)
            }
            PROF_END(PH_RAYSTEP, nTracing);
          };
          const int idleNow = 64 - nBack;   // (a service phase has handed rays out)
          // (lanes still idle after a service phase and rays left to make ready or to hand out: no step with a wave part
          // full, the next pass expands / serves again first -- as a `continue` after the service phase did, without its back edge)
          const bool fillFirst = serve && idleNow >= liThr && (ringRays > 0 || readyNow > 0);
          if (!fillFirst) {
            ray_step();
            if (liThr - idleNow > kStepAhead) ray_step();
#if I3RC_THIRD_STEP < 64
            if (liThr - idleNow > kStepAhead + I3RC_THIRD_STEP) ray_step();
#endif
          }
        }
        // what the photons' rays derive from their directions is worked out again here, so that those eleven registers per
        // lane are free during the ray loop (the radiance kernels then fit five waves per SIMD)
        r.set_direction<ZERO_IS_SLOW>(L);
      }
    }
    // ================================================================================================ PHOTON MODE
    // ---------------------------------------------------------------- EVENT phase
    // Two kinds of lanes wait for it: photons with an interaction due (scattering, reflection) and TURNOVER lanes, whose
    // photon has ended (left through the top, reached a black surface, dropped by the tracer) or that have none yet.
    // Closing a photon and starting the next one is a third of the event phase's instructions and in most event phases
    // two or three lanes need it: turnover lanes therefore sit out until kTurnMin of them have gathered (or kTurnForce
    // of them call for an event phase of their own, or nothing else is left to do).
    // (The specialised flux kernels of plain launches make their photons' starts a wavefront at a time -- STORE, part B -- and a
    // turnover lane there closes its photon and reads four words: their quorum is a pair of knobs of its own, tuning.hpp.)
    const bool wantScat = st == ST_EVENT;
    // (STORE: the three states as ONE compare, so that the ballot below is that compare's own mask -- the three-way OR came out as
    // a lane mask turned into 0 / 1 in a vector register and compared again: six vector instructions at every pass of the loop)
    constexpr unsigned kTurnStates = (1u << ST_EXIT) | (1u << kStDropped) | (1u << ST_NEW);
    // (round 16, TURN_RANGE: ... in the STORE kernels' own numbering, where the three states are the last three, it is one compare indeed)
    const bool wantTurn = TURN_RANGE ? st >= ST_NEW
                                     : (STORE ? ((kTurnStates >> (unsigned)st) & 1u) != 0u : (st == ST_EXIT || st == kStDropped || st == ST_NEW));
    const unsigned long long scMask = __ballot(wantScat), tuMask = __ballot(wantTurn);
    const unsigned long long trMask = __ballot(st == ST_TRACE);
    if constexpr (!PASS_BITS)
    if (scMask == 0ull && tuMask == 0ull && trMask == 0ull) break;   // (no photons left; any ray work has been done in ray mode above)
    int nSc = (int)__popcll(scMask), nTu = (int)__popcll(tuMask);
    // (STORE: the counts are 32-bit scalars from here on -- left as the 64-bit population counts they come from, their comparisons
    // with the quorums came out as v_cmp_gt_u64 on scalar pairs, two vector instructions of the expensive class at every pass)
    if constexpr (STORE) asm volatile("" : "+s"(nSc), "+s"(nTu));
    // (round 16: stop, runEvent and doTurn as the bits of one 32-bit scalar -- pass_decision.hpp; as booleans each wave-uniform compare
    // came out as s_cmp + s_cselect_b64 -1 / 0, joined as lane masks and copied to vcc: 24 scalar instructions in front of the step)
    int pass = 0;
    if constexpr (PASS_BITS || TURN_WORD) pass = pass_decision<kTurnMin, kTurnForce>(nSc, nTu, trMask == 0ull, evThr);
    bool runEvent;
    if constexpr (PASS_BITS) {
      // (the loop still ends HERE, in front of the event branch: left from inside that branch -- a wave that stops has the event bit set --
      // it had a second way out, and the compiler kept the photon in one register set at the head and another at the latch: twelve
      // vector copies per step and seven spilled vector registers)
      if ((pass & kPassStop) != 0) break;   // (no photons left)
      runEvent = (pass & kPassEvent) != 0;
    } else {
      runEvent = nSc + nTu > 0 && (nSc >= evThr || nTu >= kTurnForce || trMask == 0ull);
    }
    const bool doTurn = TURN_WORD ? (pass & kPassTurn) != 0 : (nTu >= kTurnMin || trMask == 0ull || nSc == 0);
    bool wantEvent = wantScat || (doTurn && wantTurn);
    unsigned long long evMask = __ballot(wantEvent);            // the lanes this event phase serves
    if (DEFER && runEvent && (DIRECT ? kReady - (int)(rdTail - rdHead) : (int)(P.rayQueueCap - (int)(qTail - qHeadEv))) < nSc) {
      // every lane of the event phase may push one record: without room for all of them the rays are served first
      wantSlots = true;
      runEvent = false;
      if (trMask == 0ull) continue;
    }
    if (runEvent) {
      unsigned long long turnAll = doTurn ? ~0ull : 0ull;   // (the wave-uniform doTurn as a mask: no branch, no detour through a vector register)
      if constexpr (TURN_WORD) {
        // (round 16: ... as a real 64-bit word, all ones or none -- the decision's bit moved up to the sign and brought down again, opaque in
        // between: seen through, every `mask & turnAll` came out as s_and_b64 with exec and two s_cselect_b32 ..., 0.  The lanes this
        // phase serves are then scalar arithmetic on the head's masks, and a lane's own flag is its bit of that mask.  Made HERE: the
        // compiler does not move the opaque step, and in front of the branch it ran at every pass)
        int sign = (int)((unsigned)(pass & kPassTurn) << 29);
        static_assert(kPassTurn == 4, "the shift above puts kPassTurn into the sign");
        if constexpr (!PASS_BITS) sign = __builtin_amdgcn_readfirstlane(sign);   // (a measurement build: beside the boolean head the compiler takes the bit for a lane's)
        asm volatile("" : "+s"(sign));
        turnAll = (unsigned long long)(long long)(sign >> 31);
        evMask = scMask | (tuMask & turnAll);
        wantEvent = __builtin_amdgcn_inverse_ballot_w64(evMask);
      }
      // The event phase reads the problem through a pointer into the kernarg segment (scalar loads where they are
      // needed) instead of keeping some sixty more values in scalar registers through the whole kernel: the kernel
      // wanted well over twice the scalar registers there are, and every spilled one comes back as a v_readlane,
      // a vector instruction, inside the voxel-step loops.  The step phases use the kernel argument itself.
      const ColdArgs ke = cold_args();
      const auto &Pe = ke->P;
      const auto &Ae = ke->A;
      if constexpr (LANE_COUNTS) {   // a 16-bit count about to overflow (one event adds at most one to each): hand over now
        // (steps: a hand-over sums the lanes' counts across the wave in 32 bits -- 64 lanes of less than 2^25 each)
        const bool full = LanePairs::about_to_overflow(accA, accB) || accSteps >= (1u << 25);
        if (__ballot(full) != 0ull) flush_lanes(full);
      }
      double *laneBlk = nullptr;
      if constexpr (BATCHED) laneBlk = lane_block(rng.batch);
      const Tally<ColdProblem, BATCHED> tally{Pe, L, laneBlk};
      PROF_BEGIN();
      // a photon that has arrived at its optical depth makes the last advance of its trace here (trace_step_lazy / finish_arrival):
      // once per event instead of a division at every voxel step
      if constexpr (TRACK) {   // ... and its length is the last piece of the segment: in the cell the photon stands in, with the weight before the scattering
        if (wantEvent && st == ST_EVENT && arrival_pending(r)) {
          float part = 0.0f;
          finish_arrival<true>(r, &part);
          track_add(trackSums, extra_block(tally.base(), Pe.oCnt), cell_index(Pe, r.ix, r.iy, r.iz), Pe.nx * Pe.ny * Pe.nz, w, part);
        }
      } else if constexpr (PATH_REG) {   // ... or the last piece of the photon's path so far
        if (wantEvent && st == ST_EVENT && arrival_pending(r)) {
          float part = 0.0f;
          finish_arrival<true>(r, &part);
          pathLen += (double)part;
        }
      } else
      if (wantEvent && st == ST_EVENT && arrival_pending(r)) finish_arrival(r);
      // ... and one that has left the grid gets its height (finish_exit).  (The general kernels do that where the step ends: here it
      // cost them nine spilled vector registers -- and with max cross-section the layer index says nothing about the height.)
      if (!GENERAL && wantEvent && (st == ST_EVENT || st == ST_EXIT)) finish_exit(Pe, r);
      // ---- part A: endings that need no random number -- tracer drop, exit through the top, arrival at a black
      //      surface -- are tallied first so that the lanes can be given their next photon before the wave
      //      generates its random block (part C), which then serves old and new photons in one go.
      // STORE: parts A and B serve turnover lanes and photons that arrive at the top or at the surface; an event phase without either
      // -- a wave-uniform fact, known here -- skips both behind ONE scalar branch, its ending counters and the hand-out included.
      // The wave's counts are taken from the masks of the two height compares themselves, joined by scalar arithmetic with the state
      // masks of the loop's head: the ballot of a flag that is an AND of compares came out as mask -> 0 / 1 in a vector register ->
      // mask, once per counter.  (Uniform control flow: a lane's bit in a compare's mask is the lane's own flag.)
      bool turnPhase = true;
      unsigned long long geTop = 0ull, leSurf = 0ull;      // STORE: lanes at or above the top / at or below the surface, any state
      unsigned long long topMask = 0ull, surfMask = 0ull;  // STORE: the lanes part A finds at the top / at the surface (none in a phase that skips it)
      if constexpr (STORE) {
        geTop = __ballot(r.z >= Pe.zMax); leSurf = __ballot(r.z <= surfaceZ);
        turnPhase = (TURN_WORD ? (tuMask & turnAll) != 0ull : (doTurn && tuMask != 0ull)) || (scMask & (geTop | leSurf)) != 0ull;
      }
      if (turnPhase) {
      const bool isEv = wantEvent && (st == ST_EVENT || st == ST_EXIT);
      const bool dropped = wantEvent && st == kStDropped;                 // :488-489
      const bool atTop = isEv && r.z >= Pe.zMax;                           // :499-514
      const bool atSurface = isEv && !atTop && r.z <= surfaceZ;           // :515-531
      const bool atBlack = atSurface && blackSurface;                     // ... and :560-562
      if constexpr (LEVELS) {
        // the segment that has just ended crosses every level between the layer it began in and the one it arrived in (a dropped
        // photon's segment tallies nothing).  The layers are the tracer's; an arrival that the tests above take for the top or the
        // surface ends on that level, so that levelFluxUp[nz] / levelFluxDown[0] get what fluxUp / fluxDown get below.
        if (isEv)
          tally_level_crossings(Pe, L, extra_block(tally.base(), Pe.oCnt), r.x, r.y, atTop ? Pe.zMax : r.z, r.dx, r.dy, r.dz, izFrom,
                                atTop ? Pe.nz + 1 : (atSurface ? 0 : r.iz), (r.iy - 1) * Pe.nx + (r.ix - 1), r.ix, r.iy, w);
      }
      if constexpr (STORE) {
        const unsigned long long evExit = scMask | (__ballot(st == ST_EXIT) & turnAll);   // isEv, as a mask
        topMask = evExit & geTop;
        surfMask = evExit & ~topMask & leSurf;
        wc.dropped += (unsigned)__popcll(__ballot(st == kStDropped) & turnAll);
        wc.top += (unsigned)__popcll(topMask);
        wc.surf += (unsigned)__popcll(surfMask);
      } else {
        wc.dropped += count_lanes(dropped);
        wc.top += count_lanes(atTop);
        wc.surf += count_lanes(atSurface);
      }
      if constexpr (BATCHED) {
        if constexpr (LANE_COUNTS) accB.add(atSurface, atTop);
        if (dropped) {
          double *const c = counter_block(rng.batch);
          unsafeAtomicAdd(c + I3RC_CNT_DROPPED, 1.0);
          unsafeAtomicAdd(c + I3RC_CNT_TRACER_CALLS, 1.0);
        }
      }
      if (dropped || atTop || atBlack) {
        // one merged branch for the three endings: a single tally atomic and a single bookkeeping block
        if (!dropped) {
          if (!rayTracing) {   // max cross-section: step back to the boundary (:504-511, :521-528)
            const float zB = atTop ? Pe.zMax : Pe.z0;
            r.x = make_periodic(r.x - r.dx * fabsf((r.z - zB) / r.dz), Pe.x0, Pe.xMax);
            r.y = make_periodic(r.y - r.dy * fabsf((r.z - zB) / r.dz), Pe.y0, Pe.yMax);
            find_xy<GENERAL>(Pe, L, r.x, r.y, r.ix, r.iy);
          }
          const int c2 = (r.iy - 1) * Pe.nx + (r.ix - 1);
          tally.boundary(atTop, c2, w);
          if constexpr (BINS) bin_add(bins, Pe.dirCos, extra_block(tally.base(), Pe.oCnt), atTop, w, pathLen);
          else if constexpr (PATH) path_add(extra_block(tally.base(), Pe.oCnt), Pe.nx * Pe.ny, atTop, c2, w, pathLen);
          if (REPLAY) { fateCol = c2; fateW = w; }
        }
        if (REPLAY) {
          order += atBlack ? 1 : 0;
          fate = dropped ? 3 : (atTop ? 0 : 1);
        }
        if (MERGE && pendCell >= 0) { tally.absorbed_sum(pendCell, pendSum); pendCell = -1; }
        close_photon();
        st = ST_NEW;
      }
      // ---- part B (uniform): hand out photon indices from the wave's reservoir
      const bool isNew = wantEvent && st == ST_NEW;
      const unsigned long long newMask = STORE ? (scMask | (tuMask & turnAll)) & __ballot(st == ST_NEW) : __ballot(isNew);
      if constexpr (BATCHED) {
        if (newMask != 0ull) {
          int need = __popcll(newMask);
          int rank = lanes_below(newMask);
          long long mine = -1;
          unsigned mineBatch = 0u;
          for (;;) {   // (uniform; a batch's last chunk may be short of `need`: then the next chunk serves the rest)
            const long long left = res.end - res.next;
            const int avail = left > 0 ? (left < 64 ? (int)left : 64) : 0;
            const int take = avail < need ? avail : need;
            if (isNew && mine < 0 && rank >= 0 && rank < take) { mine = res.next + rank; mineBatch = res.batch; }
            res.next += take; resTaken += (unsigned)take; wc.photons += (unsigned)take;
            need -= take; rank -= take;
            if (need == 0 || res.end < 0) break;
            if ((++refills & 3u) == 0u || wc.steps > 0x40000000u) flush_counters();   // (re-fits the thresholds; the counts go per lane)
            else adapt_thresholds();
            const unsigned oldBatch = res.batch;
            res.refill_batched();
            if (res.end < 0 || res.batch != oldBatch) hand_over_taken(oldBatch);
          }
          // a lane whose next photon belongs to another batch hands over what it has counted for the batch it leaves
          if constexpr (LANE_COUNTS) {
            const bool leaves = isNew && mine >= 0 && mineBatch != rng.batch && (accSteps | accA.word | accB.word | rng.used) != 0u;
            if (__ballot(leaves) != 0ull) flush_lanes(leaves);
          }
          if (isNew) {
            if (mine < 0) st = kStDone;   // (only when the launch has no chunks left)
            else rng.start((uint64_t)(Ae.firstPhoton + mine), mineBatch);
          }
        }
      } else if constexpr (STORE) {
        // The specialised flux kernels: a Directional photon's start is its stream's block 0 and nothing else -- words 0 and 1 its
        // position, word 2 its first optical depth; start layer and direction are the wave's.  Worked out where a lane turns over, that
        // is a third of the event phase's instructions for the two or three lanes that need it.  Here the WAVE works it out, for the
        // next photon numbers of its reservoir, all lanes at once (uniform control flow: this is part B), into its start store; a
        // lane that turns over reads its photon's slot.  Photons are counted where they are handed to lanes.  The reservoir is refilled
        // when it is EMPTY and more are wanted -- the other kernels refill as soon as it is short of a request, so the hand-overs
        // (flush_counters at every fourth refill, adapt_thresholds at the others: the same rule, without the shadow-step term that is
        // always zero here) fall at slightly other moments; they only schedule.  Only photons that exist are made: a launch ends with
        // every slot taken.
        if (newMask != 0ull) {
          int need = __popcll(newMask);
          int rank = lanes_below(newMask);
          long long mine = -1;
          // FLIGHT: the launch lands its photons in the fill (wave-uniform), and what this lane's slot says of its photon -- the landing
          // layer, 0 for "through the bottom", kFlightNotLanded for a photon that flies as before (first_flight.hpp)
          // (the code travels in r.iz, which every new photon's start sets anyway: a register of its own was one too many)
          bool flightLaunch = false;
          if constexpr (FLIGHT) flightLaunch = (Pe.eventFlags & kFirstFlight) != 0u;
          for (;;) {   // (uniform: from the store; when that is short, a fill -- after a refill where the reservoir is empty -- and the rest)
            const int take = need < startAvail ? need : startAvail;
            if (isNew && mine < 0 && rank >= 0 && rank < take) {
              mine = res.next - startAvail + rank;   // (the store holds the startAvail photons in front of res.next)
              if constexpr (FLIGHT) {
                if (flightLaunch) {   // (the same four words, the index word in the landing's packing; a landed slot's last word is its height)
                  const lds_float *const slot = startSlots + kStartWords * ((unsigned)mine & (unsigned)(kStartSlots - 1));
                  const int cellWord = __float_as_int(slot[StartSlot::kCell]);
                  r.x = slot[StartSlot::kX]; r.y = slot[StartSlot::kY]; r.target = slot[StartSlot::kDepth];
                  r.ix = flight_ix(cellWord); r.iy = flight_iy(cellWord); r.iz = flight_code(cellWord);
                } else {
                  const StartSlot::Words s = StartSlot::load(startSlots + kStartWords * ((unsigned)mine & (unsigned)(kStartSlots - 1)));
                  r.x = s.x; r.y = s.y; r.ix = s.ix; r.iy = s.iy; r.target = s.depth;
                }
              } else {
              const StartSlot::Words s = StartSlot::load(startSlots + kStartWords * ((unsigned)mine & (unsigned)(kStartSlots - 1)));
              r.x = s.x; r.y = s.y; r.ix = s.ix; r.iy = s.iy; r.target = s.depth;   // (the rest of the start: part C)
              }
            }
            startAvail -= take;
            wc.photons += (unsigned)take;                         // numPhotonsProcessed :459
            need -= take; rank -= take;
            if (need == 0) break;
            long long end = startState.end();
            if (res.next >= end) {
              // (the other kernels' test: a reservoir that ends where the launch ends was the last one -- no further visit of the work counter)
              if (end >= cold_args()->A.nPhotons) break;
              unsigned refilled = (unsigned)__builtin_amdgcn_readfirstlane(startState.w[WaveStartState::kRefills]) + 1u;
              // (FLIGHT: the count modulo four in the word's low two bits, the landed steps since the last hand-over above them)
              if constexpr (FLIGHT) refilled = ((refilled - 1u) & ~3u) | (refilled & 3u);
              startState.w[WaveStartState::kRefills] = (int)refilled;
              if ((refilled & 3u) == 0u || wc.steps > 0x40000000u || (FLIGHT && refilled > 0x80000000u)) flush_counters();
              else adapt_thresholds();
              res.refill();
              end = res.end;
              startState.save_end(end);
              if (res.next >= end) break;                         // (the launch has no photons left; end == nPhotons now)
            }
            // ---- the fill: one photon per lane, the operations of every other kernel's start (part C below) in their order.  A short
            // last chunk makes fewer than kStartSlots photons: the lanes beyond them work on slots that are never handed out.
            // (The problem's origin, extent and cell sizes are read where they are used, x and y one after the other: asked for all
            // at once, beside the round keys, they cost the kernels four more spilled scalar registers.)
            const long long left = end - res.next;
            const int n = left < (long long)kStartSlots ? (int)left : kStartSlots;
            {
              const long long i = res.next + (long long)(threadIdx.x & 63);
              const Philox4 o = rng.first_block_of((uint64_t)(cold_args()->A.firstPhoton + i));
              const float px = u32_to_unit_float(o.v[0]);
              float py = u32_to_unit_float(o.v[1]);
#ifdef I3RC_EXPERIMENT_SLAB   // measurement only (tools/locality_experiment.py): all photons start in one eighth of the domain
              py *= 0.125f;
#endif
              const float depth = -fast_log(fmaxf(kTiny, u32_to_unit_float(o.v[2])));
              float x, y;
              int ci, cj;
              {   // findXYIndicies :1359-1369 with the division by the (uniform) cell size done by reciprocal
                const auto &Px = cold_args()->P;
                x = Px.x0 + px * (Px.xMax - Px.x0);
                ci = min((int)exact_div(x - Px.x0, Px.deltaX, refined_rcp(Px.deltaX)) + 1, Px.nx);
                if (fabsf(L.xE[ci] - x) < spacingf(x)) ci = ci + 1;
                ci = ci == Px.nx + 1 ? 1 : ci;
              }
              {
                const auto &Py = cold_args()->P;
                y = Py.y0 + py * (Py.yMax - Py.y0);
                cj = min((int)exact_div(y - Py.y0, Py.deltaY, refined_rcp(Py.deltaY)) + 1, Py.ny);
                if (fabsf(L.yE[cj] - y) < spacingf(y)) cj = cj + 1;
                cj = cj == Py.ny + 1 ? 1 : cj;
              }
              StartSlot::store(startSlots + kStartWords * ((unsigned)i & (unsigned)(kStartSlots - 1)), x, y, ci, cj, depth);
            }
            if constexpr (FLIGHT) {
              // THE LANDING (first_flight.hpp): a zenith sun's photon goes straight down its start column until its first event, and the
              // column's table says in which step its optical path passes its depth.  A pass of its own over the slot just written,
              // read back from LDS: beside the Philox block the search did not fit the registers (fourteen spilled).  Not landed -- the
              // slot's words as before, the code kFlightNotLanded --: a photon within two spacings of its forward x or y edge (the step's
              // proximity rule would move its index after the first step and send it down the neighbouring column), and a landed height
              // that the event phase would not take for a scattering.  The steps the tracer would have counted are summed apart from
              // the wave's own count, which stays what it executed (adapt_thresholds), and join it where the counters are handed over.
              if (flightLaunch) {
                asm volatile("" ::: "memory");   // (the slot's words from LDS, not from the registers that made them)
                lds_float *const slot = startSlots + kStartWords * (((unsigned)res.next + (threadIdx.x & 63u)) & (unsigned)(kStartSlots - 1));
                const int cell = __float_as_int(slot[StartSlot::kCell]);
                const int ci = cell & ((1 << StartSlot::kIyShift) - 1), cj = (int)((unsigned)cell >> StartSlot::kIyShift);
                unsigned long long nearMask;
                {
                  const float x = slot[StartSlot::kX], y = slot[StartSlot::kY];
                  nearMask = __ballot((fabsf(L.xE[ci] - x) <= two_spacingf(x)) | (fabsf(L.yE[cj] - y) <= two_spacingf(y)));
                }
                const auto &Pf = cold_args()->P;
                const float depth = slot[StartSlot::kDepth];
                const float *const table = Pf.dirCos;
                const unsigned row = (__umul24((unsigned)(cj - 1), (unsigned)Pf.nx) + (unsigned)(ci - 1)) * (unsigned)(Pf.nz + 1);
                const int layer0 = __builtin_amdgcn_readfirstlane(startState.w[WaveStartState::kLayer]);
                const float zTop = Pf.zMax;
                const float zFrom = Pf.z0 + (1.0f - spacingf(1.0f)) * (zTop - Pf.z0);
                const FlightLanding f = first_flight_landing(
                    [table, row](int k) { return *(const float *)((const char *)table + ((row + (unsigned)k) << 2)); }, [&](int iz) { return cell_extinction<GRID>(Pf, L, ci, cj, iz); }, L.zE, zFrom,
                    layer0, -1.0f, depth, [](float rest, float e) {   // (finish_arrival's quotient)
                      float part = exact_div(rest, e, refined_rcp(e));
                      if (__builtin_expect(e < 1e-20f, 0)) part = rest / e;
                      return part;
                    });
                const bool bottom = f.layer == kFlightBottom;
                const bool lands = !__builtin_amdgcn_inverse_ballot_w64(nearMask) && (bottom || first_flight_lands(f.z, surfaceZ, zTop));
                slot[StartSlot::kCell] = __int_as_float(flight_pack(ci, cj, lands ? f.layer : kFlightNotLanded));
                if (lands && !bottom) slot[StartSlot::kDepth] = f.z;
                // (the wave's sum bit by bit from ballots -- a lane's steps are at most kFlightMaxLayers, ten bits --, a scalar: a shuffle
                // reduction's six lane addresses were hoisted out of the photon loop into six vector registers of their own)
                const uint32_t mySteps = lands && (int)(threadIdx.x & 63) < n ? (uint32_t)f.steps : 0u;   // (only photons that exist)
                uint32_t landedSteps = 0u;
                static_assert(kFlightMaxLayers < (1 << 10), "a lane's landed steps fit ten bits");
#pragma unroll
                for (int b = 0; b < 10; ++b) landedSteps += (uint32_t)__popcll(__ballot(((mySteps >> b) & 1u) != 0u)) << b;
                // (kept in the upper thirty bits of the wave's refill word -- the refills are counted modulo four -- and handed over with the
                // wave's counters: one atomic per fill, from every wave of the chip on the counters' one line, cost the step cloud 17 %)
                startState.w[WaveStartState::kRefills] = (int)((unsigned)__builtin_amdgcn_readfirstlane(startState.w[WaveStartState::kRefills]) + (landedSteps << 2));
              }
            }
            __builtin_amdgcn_wave_barrier();   // (the slots are read by other lanes of this wave: no reordering across the fill)
            res.next += n;
            startAvail = n;
          }
          if (isNew) {
            if (mine < 0) st = kStDone;
            else RngInit<Rng>::start(rng, Ae, mine);
          }
          if constexpr (FLIGHT) {
            // A lane that takes a LANDED photon: the photon stands where its first flight ended.  Its stream goes on with block 1 --
            // block 0's three deviates (position, depth) were the fill's and are counted here -- so that the block part C makes in this
            // same phase is its first scattering's, and the lane scatters now, as ST_EVENT; a photon that crossed the whole column is
            // what the step leaves below the grid -- layer 0, ST_EXIT over a black surface, else ST_EVENT -- and sits this phase's
            // part C out: finish_exit and part A serve it at its next visit.  Neither enters the ST_TRACE arm for its first flight.
            // (These scatterings are not in the head's scMask: counted here, from the one compare's mask.)
            if (flightLaunch) {
              const bool taken = isNew && mine >= 0;
              const bool landed = taken && r.iz != kFlightNotLanded;
              const bool scatters = taken && (unsigned)(r.iz - 1) < (unsigned)(kFlightNotLanded - 1);
              wc.scat += (unsigned)__popcll(__ballot(scatters));
              if (landed) {
                rng.block = 1u;
                rng.count_draws(3u);
                r.dx = Ae.solarDx; r.dy = Ae.solarDy; r.dz = Ae.solarDz;
                order = 0;
                w = 1.0f;
                r.z = r.target; r.target = 0.0f;   // (the slot's last word: the landed height; no arrival is pending)
                st = scatters ? ST_EVENT : (blackSurface ? ST_EXIT : ST_EVENT);
                wantEvent = scatters;
              }
            }
          }
        }
      } else
      if (newMask != 0ull) {
        int need = __popcll(newMask);
        int rank = lanes_below(newMask);
        long long mine = -1;
        long long avail = res.end - res.next;
        const bool slabs = SLABS && Ae.slabIds != nullptr;
        if (avail < (long long)need && (slabs ? res.end >= 0 : res.end < Ae.nPhotons)) {   // drain the reservoir, then refill it (chunk >= 64 covers the rest)
          if (isNew && rank < (int)avail) mine = res.next + rank;
          wc.photons += (unsigned)avail;                        // numPhotonsProcessed :459
          need -= (int)avail;
          rank -= (int)avail;
          // the counters go to the tally buffer (and the thresholds are re-fitted) at every fourth refill: the nine
          // atomics of a hand-over all go to the same nine addresses, from every wave of the chip
          if ((++refills & 3u) == 0u || wc.steps > 0x40000000u || wc.shadow > 0x40000000u) flush_counters();
          else adapt_thresholds();
          if (slabs) res.refill_slabs(&slabsTried[threadIdx.x >> 6]); else res.refill();
          avail = res.end - res.next;
        }
        const int taken = (int)(avail < (long long)need ? avail : (long long)need);   // < need only when the batch is exhausted
        if (isNew && mine < 0 && rank >= 0 && rank < taken) mine = res.next + rank;
        res.next += taken;
        wc.photons += (unsigned)taken;
        if (isNew) {
          if (mine < 0) st = kStDone;
          else {
            if (slabs) mine = (long long)Ae.slabIds[mine];   // position in the sorted list -> photon number
            if constexpr (!BATCHED) RngInit<Rng>::start(rng, Ae, mine);
            if (NEED_PID) pid = mine;
          }
        }
      }
      }   // (turnPhase)
      // ---- part C: one random block per lane for this event, then the event itself
      bool didScatter = false, didRoulette = false, startedTrace = false;   // per-lane flags -> wave counters below
      bool fromStore = false;                                               // STORE: this lane's photon starts here, from its slot
      if (wantEvent && st != kStDone) {
        rng.begin_event();
        if constexpr (STORE) {
          // (position, cell and optical depth came from the slot in part B; the block just made is the photon's block 0 once more -- the
          // stream goes on with block 1 -- and its three deviates are counted here and at path() below)
          if (st == ST_NEW) {
            rng.count_draws(2u);
            r.dx = Ae.solarDx; r.dy = Ae.solarDy; r.dz = Ae.solarDz;
            order = 0;
            w = 1.0f;
            r.z = Pe.z0 + (1.0f - spacingf(1.0f)) * (Pe.zMax - Pe.z0);
            r.iz = startState.w[WaveStartState::kLayer];
            fromStore = true;
            st = ST_TRACE;
          }
        } else
        if (st == ST_NEW) {                                               // :453-470
          float px, py, pz;
          if (directional) {   // newPhotonStream_Directional, Code/monteCarloIllumination.f95:91-99
            px = rng.first(); py = rng.second();
#ifdef I3RC_EXPERIMENT_SLAB   // measurement only (tools/locality_experiment.py): all photons start in one eighth of the domain
            py *= 0.125f;
#endif
            pz = 1.0f - spacingf(1.0f);
            r.dx = Ae.solarDx; r.dy = Ae.solarDy; r.dz = Ae.solarDz;
          } else {
            px = Ae.sx[pid]; py = Ae.sy[pid]; pz = Ae.sz[pid];
            make_dircos(Ae.smu[pid], Ae.sphi[pid], r.dx, r.dy, r.dz);
          }
          order = 0;
          if (REPLAY) { fate = -1; fateCol = -1; fateW = 0.0f; }
          w = 1.0f;
          if constexpr (PATH_REG) pathLen = 0.0;
          r.x = Pe.x0 + px * (Pe.xMax - Pe.x0);
          r.y = Pe.y0 + py * (Pe.yMax - Pe.y0);
          r.z = Pe.z0 + pz * (Pe.zMax - Pe.z0);
          r.ix = 1; r.iy = 1; r.iz = 1;
          if (!GENERAL && !(MULTI && !Pe.xyRegular)) {   // findXYIndicies :1359-1369 with the divisions by the (uniform) cell sizes done by reciprocal
            int i = min((int)exact_div(r.x - Pe.x0, Pe.deltaX, rcpDeltaX) + 1, Pe.nx);
            int j = min((int)exact_div(r.y - Pe.y0, Pe.deltaY, rcpDeltaY) + 1, Pe.ny);
            if (fabsf(L.xE[i] - r.x) < spacingf(r.x)) i = i + 1;
            if (fabsf(L.yE[j] - r.y) < spacingf(r.y)) j = j + 1;
            r.ix = i == Pe.nx + 1 ? 1 : i;
            r.iy = j == Pe.ny + 1 ? 1 : j;
            r.iz = izStart;
          } else {
            find_xy<true>(Pe, L, r.x, r.y, r.ix, r.iy);   // (the general kernels, and the several-components ones on an irregular x / y grid)
            find_z<true>(Pe, L, r.z, r.iz);
          }
          if constexpr (LEVELS) {   // a new photon is counted at the face of its start layer that lies behind it (a source at the top: level nz, downward)
            const bool down = !(r.dz > 0.0f);
            const int k = min(max(down ? r.iz : r.iz - 1, 0), Pe.nz), ncolL = Pe.nx * Pe.ny;
            add_global(extra_block(tally.base(), Pe.oCnt) + (size_t)((down ? Pe.nz + 1 : 0) + k) * ncolL + ((r.iy - 1) * Pe.nx + (r.ix - 1)), w);
          }
          st = ST_TRACE;
        }
        if (st == ST_EVENT) {
          if (r.z <= surfaceZ) {                                          // :515-580
            order++;
            if (!rayTracing) {
              r.x = make_periodic(r.x - r.dx * fabsf((r.z - Pe.z0) / r.dz), Pe.x0, Pe.xMax);
              r.y = make_periodic(r.y - r.dy * fabsf((r.z - Pe.z0) / r.dz), Pe.y0, Pe.yMax);
              find_xy<GENERAL>(Pe, L, r.x, r.y, r.ix, r.iy);
            }
            r.iz = 1;
            r.z = surfaceZ;
            const int c2 = (r.iy - 1) * Pe.nx + (r.ix - 1);
            tally.down(c2, w);
            if constexpr (BINS) bin_add(bins, Pe.dirCos, extra_block(tally.base(), Pe.oCnt), false, w, pathLen);   // (the weight before the reflection, the path up to here)
            else if constexpr (PATH) path_add(extra_block(tally.base(), Pe.oCnt), Pe.nx * Pe.ny, false, c2, w, pathLen);   // (likewise)
            if (REPLAY) { fateCol = c2; fateW = w; }
            float mu = exact_sqrt(rng.first());
            while (!(fabsf(mu) > 2.0f * kTiny)) mu = exact_sqrt((GENERAL || MULTI) ? rng.next() : rng.fresh());   // :546-549
            const float turn = rng.second();                               // phi = 2 pi turn (:550)
            if (useBDRF) w = w * surface_reflectance(Pe, r.x, r.y);
            else w = w * Pe.albedo;
            if (w <= kTiny) { if (REPLAY) fate = 1; st = ST_NEW; }
            else {
              if (REPLAY) make_dircos(mu, (2.0f * kPi) * turn, r.dx, r.dy, r.dz);
              else {
                // production streams: the hardware sine / cosine take their argument in revolutions -- two instructions
                // instead of the ~180 of libm's sinf + cosf (argument reduction for any float), as for the scattering azimuth
                const float sinTheta = exact_sqrt(1.0f - mu * mu);
                r.dx = sinTheta * __builtin_amdgcn_cosf(turn); r.dy = sinTheta * __builtin_amdgcn_sinf(turn); r.dz = mu;
              }
              if (defer) { pendingShadow = true; wI = w; evInfo = EventInfo::kSurface; }
              else if constexpr (RPATH)
                intensity_contribution<GRID, true>(Pe, L, rng, nested, w, r.x, r.y, r.z, r.ix, r.iy, r.iz, r.dx, r.dy, r.dz, 0, order, pathLen,
                                                   extra_block(tally.base(), Pe.oCnt));
              else if (INTENSITY)
                intensity_contribution<GRID>(Pe, L, rng, nested, w, r.x, r.y, r.z, r.ix, r.iy, r.iz, r.dx, r.dy, r.dz, 0, order);
              if constexpr (LEVELS) add_global(extra_block(tally.base(), Pe.oCnt) + c2, w);   // levelFluxUp[0]: the reflected weight, where it was reflected
              st = ST_TRACE;
            }
          } else {                                                        // :581-689
            bool scatterThis = true;
            int cell = 0;
            if (!rayTracing) {
              // max cross-section never updates the cell indices after a move (:494-496 has no index search): they are
              // those of the photon's start or of its last surface hit.  A start index of nz + 1 (a photon that starts
              // within spacing() of the domain top: thin elevated domains) is outside the grid; the reference reads
              // totalExt out of bounds there.  Here: no extinction outside the grid, hence never a scattering.
              const bool inGrid = (unsigned)(r.iz - 1) < (unsigned)Pe.nz;
              cell = inGrid ? cell_index(Pe, r.ix, r.iy, r.iz) : 0;
              const float extHere = inGrid ? Pe.totalExt[cell] : 0.0f;
              scatterThis = rng.next() < extHere / Pe.maxExt;
            }
            if (scatterThis) {
              order++;
              didScatter = true;
              // :606-632 (quirk Q2 kept): a scattering in a cell without extinction steps back over the cell face.  The
              // tracer only stops inside a cell whose extinction is positive (acc + step * 0 > target cannot hold), so
              // with ray tracing the case cannot arise and the look-up is left to the max-cross-section build.
              if (!rayTracing && cell_extinction<GRID>(Pe, L, r.ix, r.iy, r.iz) <= 0.0f) {
                if (r.x - L.xE[r.ix - 1] <= 0.0f && r.dx > 0.0f) {
                  r.x = r.x - spacingf(r.x);
                  r.ix = r.ix - 1;
                  if (r.ix <= 0) { r.ix = Pe.nx; r.x = L.xE[r.ix - 1]; r.x = r.x - 2.0f * spacingf(r.x); }
                }
                if (r.y - L.yE[r.iy - 1] <= 0.0f && r.dy > 0.0f) {
                  r.y = r.y - spacingf(r.y);
                  r.iy = r.iy - 1;
                  if (r.iy <= 0) { r.iy = Pe.ny; r.y = L.xE[r.iy - 1]; r.y = r.x - 2.0f * spacingf(r.y); }
                }
                if (r.z - L.zE[r.iz - 1] <= 0.0f && r.dz > 0.0f) { r.z = r.z - spacingf(r.z); r.iz = r.iz - 1; }
              }
              // the cell's properties are read only where the domain does not share one value (see DevProblem)
              // (FLAGS: the same expression, evaluated for the launch on the host -- event_flags.hpp -- and tested as a bit: the float
              // compares of scalar operands came out as vector compares)
              bool needCell;
              if constexpr (FLAGS) needCell = (Pe.eventFlags & kNeedCell) != 0u;
              else needCell = GENERAL || MULTI || !(Pe.uniformSsa >= 0.0f) || Pe.uniformSsa < 1.0f || Pe.uniformPf < 1;
              // (STEP_BIASED: the index from cell_word -- cell_address.hpp --, its three `- 1` as one scalar constant taken off the sum)
              if (needCell) cell = (STEP_FORM & STEP_BIASED) != 0 ? (int)(cell_word(Pe.nx, Pe.ny, r.ix, r.iy, r.iz) - (unsigned)(Pe.nx * Pe.ny + Pe.nx + 1))
                                                                  : cell_index(Pe, r.ix, r.iy, r.iz);
              int comp = 1;                                               // :637-638
              // TWO components (cloud + gas, cloud + aerosol: the usual production domain): what the scattering needs of its cell comes as
              // ONE 16-byte record (DevProblem::cellRec) -- one cache line, one trip to L2 -- and the component's pair is picked when the
              // deviate has been compared, instead of one read to choose the component and then two more, from two more arrays, that wait
              // for it.  (Asking the three arrays for both components' words at once -- five reads, five lines -- was measured: 9 - 15 %
              // SLOWER on the flux workloads; it is the lines that cost.  findIndex on (/0, c1, c2/) without a first guess answers 1 or 2,
              // never 3: see below.)
              bool fromRecord = false;
              float ssaRec = 0.0f;
              int pfiRec = 0;
              if (I3RC_CELL_RECORD_READS && (GENERAL || MULTI) && !REPLAY && multiComp && Pe.cellRec != nullptr) {
                const float rc = rng.next();
                if (Pe.ncomp == 2) {
                  const uint4 rec = Pe.cellRec[cell];
                  const float c0 = __uint_as_float(rec.x), s0 = __uint_as_float(rec.y), s1 = __uint_as_float(rec.z);
                  const int p0 = (int)(rec.w & 0xffffu), p1 = (int)(rec.w >> 16);
                  const bool second = rc >= c0;
                  comp = second ? 2 : 1; ssaRec = second ? s1 : s0; pfiRec = second ? p1 : p0;
                } else {   // three components (droplets + aerosol + gas): 32 bytes of the same line
                  const uint4 a = Pe.cellRec[2 * (size_t)cell], b = Pe.cellRec[2 * (size_t)cell + 1];
                  const bool ge0 = rc >= __uint_as_float(a.x), ge1 = rc >= __uint_as_float(a.y);
                  comp = 1 + (ge0 ? 1 : 0) + (ge1 ? 1 : 0);
                  ssaRec = comp == 1 ? __uint_as_float(a.z) : (comp == 2 ? __uint_as_float(a.w) : __uint_as_float(b.x));
                  pfiRec = comp == 1 ? (int)(b.y & 0xffffu) : (comp == 2 ? (int)(b.y >> 16) : (int)b.z);
                }
                fromRecord = true;
              } else
              if (multiComp || REPLAY) {
                const float rc = rng.next();
                if (multiComp) {
                  const float *cum = Pe.cumExt + cell;
                  if constexpr (MULTI) {
                    // findIndex without a first guess answers the largest i <= size(table) - 1 with table(i) <= value (its bisection starts
                    // with upperBound = size(table) and never returns it: Code/numericUtilities.f95:234-247, pinned by
                    // tests/golden/ref_numerics.npz): with table = (/0, cumulativeExt/) that is 1 + the number of the cell's first
                    // ncomp - 1 cumulative extinctions at or below the deviate -- the last one is never looked at.  A compare chain: every
                    // lane the same ncomp - 1 independent reads, where the bisection's reads depend on one another.
                    const int nc = Pe.ncomp;
                    for (int k = 0; k < nc - 1; ++k) comp += rc >= cum[(size_t)k * ncell] ? 1 : 0;
                  } else
                  comp = find_index(rc, [cum, ncell](int k) { return k == 1 ? 0.0f : cum[(size_t)(k - 2) * ncell]; },
                                    Pe.ncomp + 1, 0);
                }
              }
              // single-scattering albedo and phase-function entry of the cell; a value shared by the whole (one-component)
              // domain comes from the kernel arguments instead of two dependent memory reads
              // (FLAGS: a launch in which nothing absorbs -- every cell shares an albedo of at least 1 -- skips the albedo and the
              // absorption behind one uniform branch)
              if (!FLAGS || (Pe.eventFlags & kNoAbsorption) == 0u) {
              float ssa;
              if ((GENERAL || MULTI) && fromRecord) ssa = ssaRec;
              else if (!GENERAL && !MULTI && Pe.uniformSsa >= 0.0f) ssa = Pe.uniformSsa;
              else if (I3RC_CELL_RECORD_READS && !GENERAL && !MULTI && !REPLAY && Pe.cellRec != nullptr) {
                // ONE component whose cells share neither albedo nor table entry (a Mie cloud: every cell its effective radius): the two as one
                // 8-byte record (the same pointer: i3rc_hip_create makes the record that fits the domain, and only where NEITHER is shared, so
                // that the kernels of the BASELINE workloads -- both shared -- never ask)
                const uint2 rec = ((const uint2 *)Pe.cellRec)[cell];
                ssa = __uint_as_float(rec.x); pfiRec = (int)rec.y; fromRecord = true;
              }
              else ssa = Pe.ssa[(size_t)(comp - 1) * ncell + cell];
              if (ssa < 1.0f) {                                           // :642-649
                const float inc = w * (1.0f - ssa);
                if (!MERGE || tally.volume_in_lds()) tally.absorbed(cell, inc);
                else {
                  if (cell != pendCell) {
                    if (pendCell >= 0) tally.absorbed_sum(pendCell, pendSum);
                    pendCell = cell; pendSum = 0.0;
                  }
                  pendSum += (double)inc;
                }
                w = w * ssa;
              }
              }   // (kNoAbsorption)
              int pfi;
              if ((GENERAL || MULTI) && fromRecord) pfi = max(pfiRec, 1);
              else if (!GENERAL && !MULTI && Pe.uniformPf >= 1) pfi = Pe.uniformPf;
              else if (!GENERAL && !MULTI && fromRecord) pfi = max(pfiRec, 1);
              else pfi = max(Pe.pfIndex[(size_t)(comp - 1) * ncell + cell], 1);   // (index 0 marks clear cells: never a table offset of -1)
              if (defer) {                                                // :654-668: pushed after this event, traced in ray mode
                pendingShadow = true; wI = w;
                inDx = r.dx; inDy = r.dy; inDz = r.dz;                     // incoming direction
                evInfo = EventInfo::pack(comp, Pe.useHybrid && order <= Pe.numOrdersOrig, pfi);
              } else if constexpr (RPATH)
                intensity_contribution<GRID, true>(Pe, L, rng, nested, w, r.x, r.y, r.z, r.ix, r.iy, r.iz, r.dx, r.dy, r.dz, comp, order, pathLen,
                                                   extra_block(tally.base(), Pe.oCnt));
              else if (INTENSITY)
                intensity_contribution<GRID>(Pe, L, rng, nested, w, r.x, r.y, r.z, r.ix, r.iy, r.iz, r.dx, r.dy, r.dz, comp, order);
              if constexpr (FLAGS) {
                // the roulette's deviate, compares and count only where the launch can play and some lane of this phase does: the block
                // had been made unconditional -- the conversion of spare() is three float64 instructions -- and masked afterwards, in
                // every event phase of launches whose weights never leave 1
                // (ROULETTE_BIT: "can play" is the launch's, made on the host -- kPlaysRoulette -- and one bit test here)
                bool canPlay;
                if constexpr (ROULETTE_BIT) canPlay = (Pe.eventFlags & kPlaysRoulette) != 0u;
                else canPlay = Pe.useRR && (Pe.eventFlags & kWeightStaysOne) == 0u;
                if (canPlay && __ballot(w < 0.5f) != 0ull) {
                  if (w < 0.5f) {
                    didRoulette = true;
                    if (rng.spare() >= w / 1.0f) w = 0.0f; else w = 1.0f;
                  }
                }
              } else
              if (Pe.useRR && w < 0.5f) {                                  // :673-680
                didRoulette = true;
                if (rng.spare() >= w / 1.0f) w = 0.0f; else w = 1.0f;
              }
              if (w <= kTiny) { if (REPLAY) fate = 2; st = ST_NEW; }
              else {
                const CompTables ct = (GENERAL || MULTI) ? load_tables(Pe.comp[comp - 1]) : load_tables(Pe.comp0);
                float cosS;
                if constexpr (RCP_ONCE) {
                  if constexpr (TBL) cosS = scattering_cosine<REPLAY>(rng.first(), (const lds_float *)L.cosTab, ct.nInv, tableRcp);
                  else cosS = scattering_cosine<REPLAY>(rng.first(), ct.invCos + (size_t)(pfi - 1) * ct.nInv, ct.nInv, tableRcp);
                } else
                if constexpr (TBL) cosS = scattering_cosine<REPLAY>(rng.first(), (const lds_float *)L.cosTab, ct.nInv, refined_rcp((float)ct.nInv));
                else cosS = scattering_cosine<REPLAY>(rng.first(), ct.invCos + (size_t)(pfi - 1) * ct.nInv, ct.nInv, refined_rcp((float)ct.nInv));
                next_direct(rng, cosS, r.dx, r.dy, r.dz);                 // :684-687
                st = ST_TRACE;
              }
            } else {
              st = ST_TRACE;
            }
          }
        }
        if (st == ST_TRACE) {                                             // :480
          // (production streams: hardware log2, within 2 ulp -- an optical depth, not a trajectory's bit pattern; the replay
          // build follows the reference's deviates with libm's logf)
          const float tau = REPLAY ? -sample_log(fmaxf(kTiny, rng.path())) : -fast_log(fmaxf(kTiny, rng.path()));
          r.acc = 0.0f;
          if constexpr (STORE) r.target = fromStore ? r.target : tau;   // (a new photon's depth is its slot's: the same word, the same logarithm)
          else r.target = tau;
          if constexpr (LEVELS) izFrom = min(max(r.iz, 1), Pe.nz);
          if (rayTracing) { startedTrace = true; r.set_direction<ZERO_IS_SLOW>(L); }
          else {                                                          // :494-496 max cross-section move
            r.x = make_periodic(r.x + r.dx * tau / Pe.maxExt, Pe.x0, Pe.xMax);
            r.y = make_periodic(r.y + r.dy * tau / Pe.maxExt, Pe.y0, Pe.yMax);
            r.z = r.z + r.dz * tau / Pe.maxExt;
            st = ST_EVENT;
          }
        }
        // a photon that died in part C (roulette, absorbing surface) is closed here and respawns at the next event phase
        if (st == ST_NEW) {
          if (MERGE && pendCell >= 0) { tally.absorbed_sum(pendCell, pendSum); pendCell = -1; }
          close_photon();
        }
      }
      if constexpr (DIRECT) {   // one radiance direction: the event becomes a ready ray here and now (make_ray), survivors only go to LDS
        if (defer) {
          bool keep = false;
          float rayWord = 0.0f, norm = 0.0f, tauFree = 0.0f, target = 0.0f;
          if (pendingShadow)
            keep = make_ray(Pe, Ae, evInfo, inDx, inDy, inDz, rng.photon_lo(), rng.photon_hi(), rng.event_block(), rng.lane_batch(), 0, rayWord, norm, tauFree, target);
          const unsigned long long madeMask = __ballot(pendingShadow), keepMask = __ballot(keep);
          if (keep) {
            ReadyRay::store(rdBase + ((rdTail + (unsigned)lanes_below(keepMask)) & (unsigned)(kReady - 1)), kReady, r.x, r.y, r.z, r.ix, r.iy, r.iz,
                            __float_as_int(rayWord), wI, norm, tauFree, target, 0.0f);
          }
          pendingShadow = false;
          const unsigned kept = (unsigned)__popcll(keepMask);
          rdTail += kept;
          raysSkipped += (unsigned)__popcll(madeMask) - kept;
        }
      } else
      if (defer) {   // push the events of this phase into the wave's ring: one record serves all D rays of an event
        const unsigned long long pushMask = __ballot(pendingShadow);
        if (pendingShadow) {
          const EventRecord<BATCHED> ev{qBase + ((qTail + (unsigned)lanes_below(pushMask)) & qMask), Pe.rayQueueCap};
          using Ev = EventRecord<BATCHED>;
          lds_float *const rec = ev.rec;
          const int cap = ev.cap;
          rec[Ev::kX * cap] = r.x; rec[Ev::kY * cap] = r.y; rec[Ev::kZ * cap] = r.z;
          rec[Ev::kIx * cap] = __int_as_float(r.ix); rec[Ev::kIy * cap] = __int_as_float(r.iy); rec[Ev::kIz * cap] = __int_as_float(r.iz);
          rec[Ev::kWeight * cap] = wI;
          rec[Ev::kInDx * cap] = inDx; rec[Ev::kInDy * cap] = inDy; rec[Ev::kInDz * cap] = inDz;
          rec[Ev::kInfo * cap] = __int_as_float(evInfo);
          rec[Ev::kPhotonLo * cap] = __uint_as_float(rng.photon_lo());
          rec[Ev::kPhotonHiOrBatch * cap] = __uint_as_float(Ev::kCarriesBatch ? rng.lane_batch() : rng.photon_hi());
          rec[Ev::kPhiloxBlock * cap] = __uint_as_float(rng.event_block());
          pendingShadow = false;
        }
        qTail += (unsigned)__popcll(pushMask);
      }
      if constexpr (LANE_COUNTS) accA.add(didScatter, didRoulette);
      // (STORE -- ray tracing, one component: a photon with an interaction due scatters unless part A found it at the top or at the surface)
      if constexpr (STORE) wc.scat += (unsigned)__popcll(scMask & ~(topMask | surfMask));
      else wc.scat += count_lanes(didScatter);
      if constexpr (ROULETTE_BIT) { if ((Pe.eventFlags & kPlaysRoulette) != 0u) wc.roul += count_lanes(didRoulette); }   // (... and whose weights can fall)
      else if constexpr (FLAGS) { if (Pe.useRR && (Pe.eventFlags & kWeightStaysOne) == 0u) wc.roul += count_lanes(didRoulette); }
      else
      if (!STORE || Pe.useRR) wc.roul += count_lanes(didRoulette);     // (STORE: only a launch that plays roulette pays for the count)
      if constexpr (!BATCHED && !STORE) wc.calls += count_lanes(startedTrace);   // (BATCHED, STORE: a batch's / launch's photon traces = its scatterings + surface arrivals + exits + drops)
      PROF_END(PH_EVENT, __popcll(evMask));
    }
    // -------------------------------------------------------------- VOXEL-STEP phase (photons)
    // (a second step in the same pass while the next event phase is some lanes away: the phase logic is paid once for
    // both.  Written out twice: a loop around the step made the whole photon loop's code worse, -17 % on the step cloud)
    auto photon_step = [&]() {
      const bool tracing = st == ST_TRACE;
      const unsigned nTracing = count_lanes(tracing);
      wc.steps += nTracing;
      PROF_BEGIN();
#ifdef I3RC_PROFILE_PHASES
      unsigned wrapAxes = 0u;
#endif
      if (tracing) {
        if constexpr (LANE_COUNTS) accSteps++;
        StepResult s;
        if constexpr (TRACK) {   // the piece of path inside the cell the photon is in before the step (a failed step and the arriving one add nothing here)
          const int cell = cell_index(P, r.ix, r.iy, r.iz);
          float len = 0.0f;
          s = trace_step_lazy<GRID, !INTENSITY, GENERAL, false, true, CHAIN>(P, L, r, true, &len);
          if (s == STEP_CONTINUE || s == STEP_EXIT) track_add(trackSums, extra_block(P.tally, P.oCnt), cell, P.nx * P.ny * P.nz, w, len);
        } else if constexpr (PATH_REG) {   // the same piece, added to the photon's path
          float len = 0.0f;
          s = trace_step_lazy<GRID, !INTENSITY, GENERAL, false, true, CHAIN>(P, L, r, true, &len);
          if (s == STEP_CONTINUE || s == STEP_EXIT) pathLen += (double)len;
        } else if constexpr (STEP_FORM != 0) {   // (STORE, round 15: the step in another spelling -- StepForm, tracer.hpp)
          StepMasks sm;
          // (the field in LDS: the bias the step reads the extinction through -- cell_address.hpp; launch-uniform, so the compiler makes it in
          // front of the loop, and opaque to it there: it otherwise takes the constant apart again and adds its pieces per step)
          sm.ldsBias = 0u;
          if constexpr ((STEP_FORM & STEP_BIASED) != 0 && GRID == GRID_LDS) { sm.ldsBias = ext_address_bias(P, L); asm("" : "+s"(sm.ldsBias)); }
#ifdef I3RC_PROFILE_PHASES
          s = trace_step_lazy<GRID, !INTENSITY, GENERAL, false, false, CHAIN, I3RC_WRAP_PER_AXIS != 0, STEP_FORM>(P, L, r, true, nullptr, &wrapAxes, &sm);
#else
          s = trace_step_lazy<GRID, !INTENSITY, GENERAL, false, false, CHAIN, I3RC_WRAP_PER_AXIS != 0, STEP_FORM>(P, L, r, true, nullptr, nullptr, &sm);
#endif
          if constexpr ((STEP_FORM & STEP_MASKS) != 0) {
            // the mapping below as ONE chain of selects on the masks the step has anyway -- arrived, above the top, below the bottom; they
            // exclude one another --, the bottom's state wave-uniform, a scalar select: the nested form came out as two compares, a
            // select and a second exec region with a compare, a mask OR and a select of its own
            int next = sm.bottom ? (blackSurface ? ST_EXIT : ST_EVENT) : ST_TRACE;
            next = sm.top ? ST_EXIT : next;
            st = sm.reach ? ST_EVENT : next;
            if constexpr (!(STEP_FORM & STEP_COLD_ERROR)) st = sm.error ? kStDropped : st;
          } else if (s != STEP_CONTINUE) {
            st = s == STEP_DONE ? ST_EVENT : (s == STEP_ERROR ? kStDropped : ((r.iz >= 1 || blackSurface) ? ST_EXIT : ST_EVENT));
          }
          if constexpr ((STEP_FORM & STEP_COLD_ERROR) != 0) {   // the step's error exit: r.acc = -2 and the dropped state, as the early exit gave them
            if (__builtin_expect(__ballot(sm.error) != 0ull, 0))
              if (sm.error) { r.acc = -2.0f; st = kStDropped; }
          }
          s = STEP_CONTINUE;   // (the state is set)
        } else
#ifdef I3RC_PROFILE_PHASES
        s = trace_step_lazy<GRID, !INTENSITY, GENERAL, false, false, CHAIN, STORE && I3RC_WRAP_PER_AXIS>(P, L, r, true, nullptr, STORE ? &wrapAxes : nullptr);
#else
        s = trace_step_lazy<GRID, !INTENSITY, GENERAL, false, false, CHAIN, STORE && I3RC_WRAP_PER_AXIS>(P, L, r, true);   // (an arrival is finished by the event phase)
#endif
        if (GENERAL && s == STEP_EXIT) finish_exit(P, r);
        // (an exit through the top, or onto a black surface, ends the photon: such lanes wait for the turnover quorum)
        if (s != STEP_CONTINUE)
          st = s == STEP_DONE ? ST_EVENT : (s == STEP_ERROR ? kStDropped : ((r.iz >= 1 || blackSurface) ? ST_EXIT : ST_EVENT));
      }
      PROF_END(PH_STEP, nTracing);
#ifdef I3RC_PROFILE_PHASES
      if constexpr (STORE) profWrap[(__ballot((wrapAxes & 1u) != 0u) != 0ull ? 1 : 0) | (__ballot((wrapAxes & 2u) != 0u) != 0ull ? 2 : 0)]++;
#endif
    };
    photon_step();
#if I3RC_PHOTON_STEP_AHEAD < 64
    if (!runEvent && evThr - nSc > kPhotonStepAhead) photon_step();
#endif
  }
#ifdef I3RC_PROFILE_PHASES
  if ((threadIdx.x & 63) == 0) {   // (diagnostic build, omega = 1 runs: the volume-absorption tally is free)
    unsafeAtomicAdd(P.tally + P.oVol + 3 * PH_KINDS, (double)(__builtin_amdgcn_s_memtime() - profStart));   // the wave's whole loop
    for (int k = 0; k < PH_KINDS; ++k) {
      unsafeAtomicAdd(P.tally + P.oVol + 3 * k, (double)profCycles[k]);
      unsafeAtomicAdd(P.tally + P.oVol + 3 * k + 1, (double)profCount[k]);
      unsafeAtomicAdd(P.tally + P.oVol + 3 * k + 2, (double)profLanes[k]);
    }
    for (int k = 0; k < 4; ++k) unsafeAtomicAdd(P.tally + P.oVol + 3 * PH_KINDS + 1 + k, (double)profWrap[k]);
  }
#endif

  // ------------------------------------------------------------------ epilogue: flush tallies + counters
  if constexpr (BATCHED) {   // what the lanes still hold for their last batches; the tallies themselves are in global memory already
    if constexpr (LANE_COUNTS) flush_lanes(true); else flush_counters();
    hand_over_taken(res.batch);
    return;
  }
  __syncthreads();
  {
    const ColdArgs ka = cold_args();   // (offsets and sizes straight from the kernarg segment: see cold_args)
    double *const out = ka->P.tally;
    if (ka->P.ldsTallies) {
      const int ncol = ka->P.nx * ka->P.ny;
      const int oUp = ka->P.oUp, oDown = ka->P.oDown;
      for (int i = threadIdx.x; i < ncol; i += blockDim.x) {
        const tally_t u = L.tUp[i], d = L.tDown[i];
        if (u != (tally_t)0) add_global(out + oUp + i, u);
        if (d != (tally_t)0) add_global(out + oDown + i, d);
      }
    }
    if (ka->P.ldsVolume) {
      const int nVol = ka->P.nx * ka->P.ny * ka->P.nz, oVol = ka->P.oVol;
      for (int i = threadIdx.x; i < nVol; i += blockDim.x) {
        const tally_t v = L.tVol[i];
        if (v != (tally_t)0) add_global(out + oVol + i, v);
      }
    }
    if constexpr (TRACK)
      if (trackSums != nullptr) {
        double *const block = extra_block(out, ka->P.oCnt);
        const int ncellT = ka->P.nx * ka->P.ny * ka->P.nz;
        for (int i = threadIdx.x; i < ncellT; i += blockDim.x) {
          const double v = trackSums[i];
          if (v != 0.0) add_global(block + i, v);
        }
      }
    if constexpr (BINS)
      if (bins.sums != nullptr) {
        double *const block = extra_block(out, ka->P.oCnt);
        for (int i = threadIdx.x; i < 4 * (bins.nBins + 1); i += blockDim.x) {
          const double v = bins.sums[i];
          if (v != 0.0) add_global(block + i, v);
        }
      }
    if (ka->P.ldsIntensity) {
      const int nInt = (ka->P.ncomp + 1) * ka->P.nDir * ka->P.nx * ka->P.ny;
      const int oInt = ka->P.oInt;
      for (int i = threadIdx.x; i < nInt; i += blockDim.x) {
        const tally_t v = L.tInt[i];
        if (v != (tally_t)0) add_global(out + oInt + i, v);
      }
    }
    // nested local-estimate work and the deviate count are per lane; everything else is already per wave
    const double nestedShadow = wave_sum((double)nested.shadow), nestedCalls = wave_sum((double)nested.calls);
    const double draws = wave_sum((double)rng.total());
    flush_counters();
    if ((threadIdx.x & 63) == 0) {
      double *const counters = out + ka->P.oCnt;
      if (nestedShadow != 0.0) unsafeAtomicAdd(counters + I3RC_CNT_SHADOW_STEPS, nestedShadow);
      if (nestedCalls != 0.0) unsafeAtomicAdd(counters + I3RC_CNT_TRACER_CALLS, nestedCalls);
      if (draws != 0.0) unsafeAtomicAdd(counters + I3RC_CNT_RNG_DRAWS, draws);
      if (raysSkipped != 0u) unsafeAtomicAdd(counters + I3RC_CNT_RAYS_SKIPPED, (double)raysSkipped);
    }
  }
}

// Test hook: independent tracer calls, one ray per thread.
// (CLEARMAP = false: domains of more than 65534 layers, whose clear-air map -- 16 bits per bound -- is not used: i3rc_hip.hip)
// (GRID: the bricked copy -- what the hook reads unless i3rc_hip_select_grid_place says otherwise --, the plain field, or the column records)
template <int GRID, bool CLEARMAP>
__global__ void __launch_bounds__(256) trace_rays_kernel(const DevProblem P, long long n, const float *dir, float *pos,
                                                         int32_t *idx, const float *target, float *tau, int32_t *steps) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Lds L;
  L.xE = (lds_float *)smem; L.yE = L.xE + P.nx + 1; L.zE = L.yE + P.ny + 1;
  L.tUp = L.tDown = L.tVol = nullptr; L.dirCos = nullptr;
  L.ext = L.zE + P.nz + 1;   // the clear-air map of the bricked field
  if (GRID == GRID_BRICKS && CLEARMAP)
    for (int i = threadIdx.x; i < P.clearNx * (((P.ny - 1) >> P.clearShift) + 1); i += blockDim.x) L.ext[i] = __uint_as_float(P.clearMap[i]);
  if (GRID == GRID_COLBASE)
    for (int i = threadIdx.x; i < P.nz; i += blockDim.x) L.ext[i] = P.colBase[i];
  for (int i = threadIdx.x; i <= P.nx; i += blockDim.x) L.xE[i] = P.xE[i];
  for (int i = threadIdx.x; i <= P.ny; i += blockDim.x) L.yE[i] = P.yE[i];
  for (int i = threadIdx.x; i <= P.nz; i += blockDim.x) L.zE[i] = P.zE[i];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Ray r;
  r.x = pos[3 * i]; r.y = pos[3 * i + 1]; r.z = pos[3 * i + 2];
  r.dx = dir[3 * i]; r.dy = dir[3 * i + 1]; r.dz = dir[3 * i + 2];
  r.ix = idx[3 * i]; r.iy = idx[3 * i + 1]; r.iz = idx[3 * i + 2];
  r.set_direction(L);
  r.acc = 0.0f;
  const bool hasTarget = target[i] >= 0.0f;
  r.target = target[i];
  int ns = 0;
  StepResult s;
  do { ns++; s = trace_step<GRID, CLEARMAP>(P, L, r, hasTarget); } while (s == STEP_CONTINUE && ns < (1 << 24));
  pos[3 * i] = r.x; pos[3 * i + 1] = r.y; pos[3 * i + 2] = r.z;
  idx[3 * i] = r.ix; idx[3 * i + 1] = r.iy; idx[3 * i + 2] = r.iz;
  tau[i] = r.acc;
  steps[i] = ns;
}

#if I3RC_FIRST_FLIGHT_TABLE != 0
// The column table of the first flight (first_flight.hpp): table[column][k], k = 0 .. nz, the optical path after k downward steps from
// the Directional start height, one thread per column -- by the tracer's own step from the kernels' own start state (x and y at the
// cell's centre: with dx = dy = 0 nothing of the step reads them but the proximity rule), towards a target it never reaches, so that the
// sums are the photon kernels' by construction.  info[0]: the start layer (the kernels' izStart); info[1] != 0: some sweep met what
// makes the table unfit -- a start layer outside the grid, a step that failed (step <= 0, a NaN), an index that moved sideways or not
// down by one, a sum that fell or is not finite -- and no launch may land photons from it.  Entries beyond the start layer repeat the
// last sum (never read).  The field is read in its plain form (DevProblem::totalExt), whatever place the photon kernels read it at:
// every packed form gives the field's words back bit for bit.
__global__ void __launch_bounds__(256) first_flight_table_kernel(const DevProblem P, float *table, int *info) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  Lds L;
  L.xE = (lds_float *)smem; L.yE = L.xE + P.nx + 1; L.zE = L.yE + P.ny + 1;
  L.tUp = L.tDown = L.tVol = nullptr; L.dirCos = nullptr; L.ext = nullptr;
  for (int i = threadIdx.x; i <= P.nx; i += blockDim.x) L.xE[i] = P.xE[i];
  for (int i = threadIdx.x; i <= P.ny; i += blockDim.x) L.yE[i] = P.yE[i];
  for (int i = threadIdx.x; i <= P.nz; i += blockDim.x) L.zE[i] = P.zE[i];
  __syncthreads();
  const int col = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (col >= P.nx * P.ny) return;
  const float zStart = P.z0 + (1.0f - spacingf(1.0f)) * (P.zMax - P.z0);
  int izStart = 1;
  find_z<true>(P, L, zStart, izStart);
  if (col == 0) info[0] = izStart;
  float *const row = table + (size_t)col * (size_t)(P.nz + 1);
  bool bad = izStart < 1 || izStart > P.nz;
  float last = 0.0f;
  row[0] = 0.0f;
  int k = 1;
  if (!bad) {
    const int ix = col % P.nx + 1, iy = col / P.nx + 1;
    Ray r;
    r.x = 0.5f * (L.xE[ix - 1] + L.xE[ix]); r.y = 0.5f * (L.yE[iy - 1] + L.yE[iy]); r.z = zStart;
    r.dx = 0.0f; r.dy = 0.0f; r.dz = -1.0f;
    r.ix = ix; r.iy = iy; r.iz = izStart;
    r.set_direction(L);
    r.acc = 0.0f; r.target = kHuge;
    for (; k <= izStart; ++k) {
      const StepResult s = trace_step_lazy<GRID_GLOBAL>(P, L, r, true);
      const bool ok = s == (k < izStart ? STEP_CONTINUE : STEP_EXIT) && r.iz == izStart - k && r.ix == ix && r.iy == iy && r.acc >= last && r.acc < kHuge;
      if (!ok) { bad = true; break; }
      last = r.acc;
      row[k] = last;
    }
  }
  for (; k <= P.nz; ++k) row[k] = last;
  if (bad) atomicOr(&info[1], 1);
}
#endif

// Test hook: exact_div / exact_sqrt against the IEEE operations they replace.
__global__ void arith_check_kernel(long long n, const float *num, const float *den, unsigned long long *mismatch) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = num[i], b = den[i];
  const float q = exact_div(a, b, refined_rcp(b)), qRef = a / b;
  if (__float_as_uint(q) != __float_as_uint(qRef)) atomicAdd(&mismatch[0], 1ull);
  const float x = fabsf(a);
  if (__float_as_uint(exact_sqrt(x)) != __float_as_uint(sqrtf(x))) atomicAdd(&mismatch[1], 1ull);
}

// Test hooks: findIndex and computeSurfaceReflectance as the photon kernels evaluate them (tracer.hpp find_index, surface_reflectance),
// one thread per value -- held against the reference's own routines (tests/golden/ref_numerics.npz) by tests/test_gpu_ref_numerics.py.
__global__ void find_index_kernel(int n, const float *table, long long m, const float *values, const int32_t *firstGuess, int32_t *out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  out[i] = find_index(values[i], [table](int k) { return table[k - 1]; }, n, firstGuess ? firstGuess[i] : 0);
}
struct SurfaceOnly { const float *xsE, *ysE, *brdf; int nxs, nys; };   // (what surface_reflectance reads of a DevProblem)
__global__ void surface_reflectance_kernel(const SurfaceOnly S, long long m, const float *x, const float *y, float *out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  out[i] = surface_reflectance(S, x[i], y[i]);
}

// Test hook: raw Philox blocks as the photon streams see them.
__global__ void philox_kernel(uint32_t seed0, uint32_t seed1, long long firstPhoton, long long n, int blocksPerPhoton,
                              uint32_t *out, float *outf) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PhiloxStream g;
  g.init(seed0, seed1);
  g.start((uint64_t)(firstPhoton + i));
  for (int b = 0; b < blocksPerPhoton; ++b) {
    const Philox4 o = philox4x32_10(g.id_lo, g.id_hi, (uint32_t)b, 0u, seed0, seed1);
    g.begin_event();   // block b of the stream, as the photon kernel draws it
    const float roles[4] = {g.first(), g.second(), g.path(), g.spare()};
    for (int k = 0; k < 4; ++k) {
      out[(i * blocksPerPhoton + b) * 4 + k] = o.v[k];
      outf[(i * blocksPerPhoton + b) * 4 + k] = roles[k];
    }
  }
}

}  // namespace i3rc

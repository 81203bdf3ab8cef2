// Where a launch is decided, on the host and without a HIP call: the facts of a problem (ProblemFacts: derive_facts from the host
// arrays, the setters, the handle's knobs), the switches of the process (EnvKnobs) and plan_launch, a pure function of both and of
// the kind of the launch.  i3rc_hip.hip fills a DevProblem from the handle and the decision and launches what it names;
// i3rc_hip_problem_facts / i3rc_hip_plan_launch hand both to the CPU suite (tests/test_launch_plan_cpu.py, against the launches
// recorded in tests/golden/launch_plans.json).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "tally_block.hpp"

namespace i3rc {

// Environment knobs (I3RC_*): a switch that is on unless set to 0, ...
inline bool env_on(const char *name) { const char *v = std::getenv(name); return !(v && std::atoi(v) == 0); }
// ... an integer with a default, ...
inline long long env_int(const char *name, long long dflt) { const char *v = std::getenv(name); return v ? std::atoll(v) : dflt; }
// ... and a pair of integers "a,b" (false where unset or not of that form)
inline bool env_pair(const char *name, int &a, int &b) { const char *v = std::getenv(name); return v && std::sscanf(v, "%d,%d", &a, &b) == 2; }

// The switches of the process that steer a launch, read once (process()); a test hands plan_launch a copy of its own.
struct EnvKnobs {
  bool columns = true;       // I3RC_COLUMNS=0: no column records on the automatic place
  bool ldsTallies = true;    // I3RC_LDS_TALLIES=0: as i3rc_hip_set_lds_tallies(h, 0), for the process
  bool tableLds = true;      // I3RC_TABLE_LDS=0: never the inverse table in LDS
  // (grid places as a bit mask: LDS, global memory and column records.  Plain launches on bricked fields: Landsat-119 -2.5 %, the
  // scene tiled 2 x 2 +10 %: left out.  Fused: Landsat-36 +13 %, radar 640 +12 %, step cloud +1.5 ... 3 % in the kernels' own time;
  // on column records +1 ... 2.5 %)
  int plainPlaces = 11;      // I3RC_TABLE_LDS_PLACES
  int fusedPlaces = 11;      // I3RC_FUSED_TABLE_LDS_PLACES
  bool direct = true;        // I3RC_DIRECT=0 keeps the event ring for one radiance direction too
  bool cellRecords = true;   // I3RC_CELL_RECORDS (DevProblem::cellRec; 0: the kernels read the plain arrays)
  bool firstFlight = true;   // I3RC_FIRST_FLIGHT_TABLE=0: no launch lands its photons from the column table (first_flight.hpp); no plan reads it
  static const EnvKnobs &process() {
    static const EnvKnobs k{env_on("I3RC_COLUMNS"), env_on("I3RC_LDS_TALLIES"), env_on("I3RC_TABLE_LDS"), (int)env_int("I3RC_TABLE_LDS_PLACES", 11),
                            (int)env_int("I3RC_FUSED_TABLE_LDS_PLACES", 11), env_on("I3RC_DIRECT"), env_on("I3RC_CELL_RECORDS"), env_on("I3RC_FIRST_FLIGHT_TABLE")};
    return k;
  }
};

// Everything the decision of a launch reads, stated once: the handle (i3rc_hip.hip) IS one of these, with its device state behind it.
struct ProblemFacts {
  int nx = 0, ny = 0, nz = 0, ncomp = 0, nDir = 0;
  // the field (derive_facts)
  int xyRegular = 0, zRegular = 0;
  float maxExt = 0.f;
  bool empty = false;        // optically empty: width * maxExt <= 1e-5 (see traced)
  bool absorbing = false;    // some cell of some component has omega < 1: launches tally volume absorption, and fluxAbsorbed is formed from it (absorbed_columns_kernel)
  float uniformSsa = -1.f;   // one-component domains: the value every cell shares, else -1
  int uniformPf = 0;         // ... and the phase-function entry every cell shares, else 0
  int cellRecBytes = 0;      // a scattering's reads of its cell as one record (DevProblem::cellRec) of 8 / 16 / 32 bytes: one / two / three components; 0: none
  bool colRecords = false;   // one record per column: every column is one run of one value (DevProblem::colRec) ...
  bool colBase = false;      // ... over a base profile (DevProblem::colBase, nz floats): the records then hold what lies ON the profile
  int bsx = 0, bsy = 0, bsz = 0, nbx = 0, nby = 0, nbz = 0;   // totalExt in bricks of 32 cells (DevProblem::extBrick)
  int clearShift = 0, clearNx = 1, clearWords = 1;            // ... and its clear-air map (DevProblem::clearMap)
  std::vector<int> maxPfIndex;
  // what the setters add
  std::vector<CompTables> comp;   // per component (sized by derive_facts): a table is present where its pointer is set
  std::vector<int> nInvEntries, nFwdEntries;
  i3rc_params params{};
  int nxs = 0, nys = 0;
  bool surfaceSet = false;   // (i3rc_hip_set_surface)
  ExtraTally extra = EXTRA_NONE;   // set_extra_tally: the block plain flux launches also fill, behind the counters (tally_block.hpp)
  int pathBins = 0;                // ... and, while it is EXTRA_PATH_BINS, the histogram's bins (i3rc_hip_set_path_histogram), else 0
  // the handle's knobs
  int kernelVariant = I3RC_KERNEL_AUTO;  // test / tuning knob (i3rc_hip_select_kernel)
  int gridPlace = I3RC_GRID_AUTO;        // test / tuning knob (i3rc_hip_select_grid_place)
  bool ldsTalliesOn = true;              // i3rc_hip_set_lds_tallies
};

inline size_t ncell_bytes(const ProblemFacts &f) { return sizeof(float) * (size_t)f.nx * f.ny * f.nz; }

inline float host_spacing(float x) {
  if (x == 0.0f) return FLT_MIN;
  int e;
  (void)std::frexp(std::fabs(x), &e);
  float r = std::ldexp(1.0f, e - 24);
  return r < FLT_MIN ? FLT_MIN : r;
}

// what the scans for column records leave behind for the upload (derive_facts; may be left out)
struct ColumnRecords { std::vector<uint32_t> rec; std::vector<float> base; };

// The facts of the field of a domain (checked by i3rc_hip_create: sizes, edges that increase, no null array), from the host arrays
// alone.  Returns the text of a refusal, or nothing.
inline std::string derive_facts(ProblemFacts &f, const EnvKnobs &env, int nx, int ny, int nz, int ncomp, const float *xEdges, const float *yEdges,
                                const float *zEdges, const float *totalExt, const float *cumExt, const float *ssa, const int32_t *pfIndex,
                                ColumnRecords *cols = nullptr) {
  f.nx = nx; f.ny = ny; f.nz = nz; f.ncomp = ncomp;
  f.comp.assign(ncomp, CompTables{}); f.nInvEntries.assign(ncomp, 0); f.nFwdEntries.assign(ncomp, 0); f.maxPfIndex.assign(ncomp, 0);
  const size_t ncell = (size_t)nx * ny * nz;
  {
    // bricks of 32 cells: 8 deep where the grid has the layers for it (photon paths and shadow rays cross z faces
    // most often in cloud fields, whose cells are flatter than wide), the rest shared by x and y
    auto log2le = [](int n, int cap) { int s = 0; while ((2 << s) <= n && s + 1 <= cap) ++s; return s; };
    f.bsz = log2le(nz, 3);
    f.bsy = log2le(ny, (5 - f.bsz) / 2);
    int bz, by;   // tuning knob: "<log2 depth>,<log2 width in y>" (the rest of the 32 cells in x)
    if (env_pair("I3RC_BRICK", bz, by) && bz >= 0 && by >= 0 && bz + by <= 5) { f.bsz = log2le(nz, bz); f.bsy = log2le(ny, by); }
    f.bsx = 5 - f.bsz - f.bsy;
    f.nbx = (nx + (1 << f.bsx) - 1) >> f.bsx; f.nby = (ny + (1 << f.bsy) - 1) >> f.bsy;
    f.nbz = (nz + 1 + (1 << f.bsz) - 1) >> f.bsz;   // (room for the layer nz + 1 of zeros, as in dExt)
    if ((int64_t)f.nbx * f.nby >= ((int64_t)1 << 24) || (int64_t)f.nbx * f.nby * f.nbz >= ((int64_t)1 << 26))
      return "i3rc_hip_create: domain too large for the bricked extinction copy";
    // clear-air map: lowest / highest layer with any extinction per footprint of 2^s x 2^s columns, at most 1024 words
    int sft = 0;
    while ((size_t)(((nx - 1) >> sft) + 1) * (size_t)(((ny - 1) >> sft) + 1) > 1024) ++sft;
    f.clearShift = sft; f.clearNx = ((nx - 1) >> sft) + 1;
    f.clearWords = f.clearNx * (((ny - 1) >> sft) + 1);
  }
  {
    ColumnRecords scratch;
    ColumnRecords &c = cols ? *cols : scratch;
    c.rec.resize(2 * (size_t)nx * ny); c.base.resize((size_t)nz);
    f.colRecords = i3rc_hip_column_records(nx, ny, nz, totalExt, c.rec.data()) == 1;
    // the same over a value per layer (a uniform gas under / around the clouds)
    if (!f.colRecords) f.colRecords = f.colBase = i3rc_hip_column_records_base(nx, ny, nz, totalExt, c.rec.data(), c.base.data()) == 1;
  }
  // regular-spacing flags, new_Integrator :193-211
  {
    const float dx = xEdges[1] - xEdges[0], dy = yEdges[1] - yEdges[0], dz = zEdges[1] - zEdges[0];
    int xy = 1, z = 1;
    for (int i = 0; i < nx; ++i) if (!(std::fabs((xEdges[i + 1] - xEdges[i]) - dx) <= 2.0f * host_spacing(xEdges[i + 1]))) xy = 0;
    for (int i = 0; i < ny; ++i) if (!(std::fabs((yEdges[i + 1] - yEdges[i]) - dy) <= 2.0f * host_spacing(yEdges[i + 1]))) xy = 0;
    for (int i = 0; i < nz; ++i) if (!(std::fabs((zEdges[i + 1] - zEdges[i]) - dz) <= host_spacing(zEdges[i + 1]))) z = 0;
    f.xyRegular = xy; f.zRegular = z;
  }
  f.maxExt = totalExt[0];
  for (size_t i = 1; i < ncell; ++i) f.maxExt = std::max(f.maxExt, totalExt[i]);  // computeRT :438-439
  // Max cross-section divides the optical depth by the largest extinction of the domain (:494-496): with no extinction
  // anywhere that is a step of infinite length and the reference's makePeriodic never returns -- nor does it once the
  // step exceeds 2^24 domain widths, where subtracting a width no longer changes a float32.  A photon in such an
  // (optically empty: width * maxExtinction <= 1e-5) domain flies straight to the boundary, which is what ray
  // tracing gives: such a domain is traced.
  f.empty = !(f.maxExt * std::min(xEdges[nx] - xEdges[0], yEdges[ny] - yEdges[0]) > 1e-5f);
  for (int c = 0; c < ncomp; ++c) {
    int m = 0;
    for (size_t i = 0; i < ncell; ++i) m = std::max(m, pfIndex[(size_t)c * ncell + i]);
    f.maxPfIndex[c] = m;
  }
  // Absorbing: some component has omega < 1 in a cell where the kernels can select it -- the rule of uniformSsa below, for several
  // components.  They pick component 1 + (the number of k < ncomp - 1 with rc >= cumExt[k]) for a deviate rc in [0, 1] -- 1.0 itself
  // included (u32_to_unit_float rounds the largest words up to it) --, so component c is selected on [cumExt[c - 1], cumExt[c]), the
  // first from below 0 and the last up to above 1: it can be selected where that interval meets [0, 1].  A component without
  // extinction in a cell is never selected there unless it is the last one, which a deviate of 1.0 selects wherever the slices before
  // it reach 1.  (So a gas that is zero in some cells with omega = 0 there does not make a conservative domain absorbing as the first
  // component, and does as the last: its omega is then used, rarely, and the absorbed weight must reach fluxAbsorbed.)
  for (size_t i = 0; i < ncell && !f.absorbing; ++i) {
    if (totalExt[i] == 0.0f) continue;
    for (int c = 0; c < ncomp && !f.absorbing; ++c) {
      const float lo = c == 0 ? -INFINITY : cumExt[(size_t)(c - 1) * ncell + i];
      const float hi = c == ncomp - 1 ? INFINITY : cumExt[(size_t)c * ncell + i];
      const bool selectable = lo <= 1.0f && hi > 0.0f && hi > lo;
      f.absorbing = selectable && ssa[(size_t)c * ncell + i] < 1.0f;
    }
  }
  if (ncomp == 1) {
    // Values that every cell WITH EXTINCTION shares travel in the kernel arguments (specialised kernels: ray tracing, where a
    // photon can only be scattered in a cell of positive extinction -- the tracer never stops in any other --, so what the
    // clear cells hold is never read: the I3RC cloud fields have omega = 0 and phase-function entry 0 there).  Without this
    // every scattering reads two more words from two more arrays of the field's size, which on the Landsat fields
    // do not fit in L2 beside it.
    bool sameSsa = true, samePf = true, any = false;
    float ssa0 = 1.f; int32_t pf0 = 1;
    for (size_t i = 0; i < ncell && (sameSsa || samePf); ++i) {
      if (totalExt[i] == 0.0f) continue;
      if (!any) { any = true; ssa0 = ssa[i]; pf0 = pfIndex[i]; continue; }
      sameSsa = sameSsa && ssa[i] == ssa0;
      samePf = samePf && pfIndex[i] == pf0;
    }
    f.uniformSsa = (sameSsa && ssa0 >= 0.f) ? ssa0 : -1.f;
    f.uniformPf = (samePf && pf0 >= 1) ? pf0 : 0;
  }
  // Cell records: one component with neither albedo nor entry shared -- {ssa, pfIndex}, 8 bytes a cell --; two or three components
  // whose first two entries fit the word they share -- 16 or 32 bytes
  if (env.cellRecords && ncomp == 1 && f.uniformSsa < 0.0f && f.uniformPf < 1) f.cellRecBytes = 8;
  if (env.cellRecords && (ncomp == 2 || ncomp == 3)) {
    bool fits = true;
    for (size_t i = 0; i < 2 * ncell && fits; ++i) fits = pfIndex[i] >= 0 && pfIndex[i] < 65536;   // (the first two entries share a word)
    if (fits) f.cellRecBytes = ncomp == 2 ? 16 : 32;
  }
  return {};
}

// Which kernel runs a launch (see photon_kernel): the common problem class -- regular grid,
// ray tracing, one component, no BRDF grid, Directional source -- has specialised kernels.
// A surface description with a single cell (new_SurfaceDescription((/ albedo /)), the form BASELINE.json's Landsat
// radiance case uses) reflects like surfaceAlbedo: computeSurfaceReflectance returns its one parameter wherever the
// photon lands (Code/surfaceProperties.f95:121-162), and the weight is multiplied by the same float.
inline bool uniform_surface(const ProblemFacts &f) { return f.params.useSurfaceBDRF && f.nxs == 1 && f.nys == 1; }

// ray tracing asked for, or max cross-section on an optically empty domain (see derive_facts)
inline bool traced(const ProblemFacts &f) { return f.params.useRayTracing || f.empty; }

inline bool common_class(const ProblemFacts &f, int srcKind) {
  const bool gridSurface = f.params.useSurfaceBDRF && !uniform_surface(f);
  return f.xyRegular && traced(f) && !gridSurface && f.ncomp == 1 && srcKind == 0;
}
// ... and the same class widened: several components (photon_kernel, MULTI; round 5).
// (... and, since the kernels that run it keep those two paths behind run-time switches, with an irregular x / y grid or a gridded surface)
inline bool multi_class(const ProblemFacts &f, int srcKind) { return traced(f) && srcKind == 0; }

// One radiance direction (nadir views: BASELINE.json's radar case): the radiance kernels without an event ring (photon_kernel,
// DIRECT).  I3RC_DIRECT=0 keeps the ring for them too.
#ifdef I3RC_NESTED_BUILD   /* measurement build: radiance problems run the general kernels with the nested local estimate (kernels.hpp) */
constexpr bool kNestedBuild = true;
#else
constexpr bool kNestedBuild = false;
#endif
inline bool direct_rays(const ProblemFacts &f, const EnvKnobs &env) {
  return env.direct && f.nDir == 1 && f.kernelVariant != I3RC_KERNEL_RING && !kNestedBuild;
}

// its stream -- what the Rng template argument of photon_kernel carries: plain (all false), fused, replay, level tally, track tally, path tally,
// path histogram, radiance path tally -- ...
struct StreamKind {
  bool replay, batched;
  ExtraTally extra;
  bool (*startStore)(bool intensity, bool general, int grid, bool multi);   // (has_start_store, kernels.hpp, of the stream's type)
};
template <class Rng>
constexpr StreamKind stream_of() { return {Rng::kReplay, Rng::kBatched, Rng::kExtra, &has_start_store<Rng>}; }
inline StreamKind plain_stream(ExtraTally extra) {   // (of a plain launch: the production stream, or the one that also fills the extra tally block)
  return extra == EXTRA_LEVELS   ? stream_of<PhiloxLevelStream>()
         : extra == EXTRA_TRACKS ? stream_of<PhiloxTrackStream>()
         : extra == EXTRA_PATHS  ? stream_of<PhiloxPathStream>()
         : extra == EXTRA_PATH_BINS ? stream_of<PhiloxBinStream>()
         : extra == EXTRA_RADIANCE_PATHS ? stream_of<PhiloxRadiancePathStream>()
                                 : stream_of<PhiloxStream>();
}
// ... and the kind of its source (i3rc_source::kind, RunArgs::srcKind)
struct LaunchKind { StreamKind stream; int srcKind; };

// A production instantiation of photon_kernel: its template arguments after the stream -- the key a launch looks it up by
struct KernelKey {
  bool intensity, general;
  int place;                 // GridPlace
  bool tbl, direct, wide;    // (the inverse table in LDS; one radiance direction without the event ring; the widened class, MULTI)
  bool operator==(const KernelKey &o) const {
    return intensity == o.intensity && general == o.general && place == o.place && tbl == o.tbl && direct == o.direct && wide == o.wide;
  }
};

constexpr size_t kLdsBudget = 64 * 1024;  // per workgroup: leaves room for >= 2 workgroups per CU
// ... which what a launch MUST have in LDS -- the edge vectors, the directions, the ray queues -- may exceed, up to the 160 KB of a
// compute unit (less the kernels' few static words): a 2-D domain of 20 000 columns runs with one workgroup per CU, slowly,
// instead of being refused
constexpr size_t kLdsHard = 158 * 1024;
// what a launch may allocate: a compute unit's LDS less the kernels' static LDS (kStaticLdsBytes, tracer.hpp: the store kernels use all of it)
constexpr size_t kLdsLaunchMax = 160 * 1024 - kStaticLdsBytes;
// the table form (photon_kernel, TBL): two workgroups of 1024 threads share a compute unit's 160 KB
constexpr size_t kLdsTableForm = 79 * 1024;
// The running estimate of a workgroup's LDS that steers the decisions: an upper bound of what the launch allocates, which is lds_plan's
// own end (lds_bytes).  take(): the region is placed if it still fits the budget.
struct LdsEstimate {
  size_t bytes;
  bool fits(size_t region, size_t budget) const { return bytes + region <= budget; }
  bool take(size_t region, size_t budget) { if (!fits(region, budget)) return false; bytes += region; return true; }
};
// the waves' start stores in a workgroup of `threads` (photon_kernel, STORE; StartSlot, tracer.hpp)
constexpr size_t start_store_bytes(int threads) { return sizeof(float) * kStartWords * kStartSlots * (size_t)(threads / 64); }

struct LaunchDecision {
  std::string refusal;       // not empty: the launch is refused with this text ...
  bool early = false;        // ... before the source is looked at (the problem is incomplete or too large), else after it (LDS)
  int place = GRID_GLOBAL;   // GridPlace: where the kernels read the extinction field; the packed form passed is the place's
  int ldsTallies = 0, ldsVolume = 0, ldsIntensity = 0, rayQueueCap = 0;
  int ldsGrid = 0;           // (bit 1, kLdsGridTrackSums: the track-length sums in LDS)
  int ldsBins = 0;           // the path histogram's sums and edges in LDS (photon_kernel, BINS; DevProblem::ldsGrid's bit 2, kLdsGridBinSums) ...
  int pathBins = 0;          // ... and its bins, which size that region (bin_region_words)
  KernelKey key{};           // (key.tbl: the inverse table in LDS)
  int threads = 256;
  bool startStore = false;   // the kernel starts its photons from per-wave start stores in LDS (photon_kernel, STORE)
  size_t startStoreBytes = 0;
  size_t estimate = 0;       // the running estimate the flags were decided with, rounded up to 16 bytes
  size_t ldsBytes = 0;       // dynamic LDS of the launch
  // what lds_plan reads of a DevProblem, for the host's call of it
  int nx = 0, ny = 0, nz = 0, ncomp = 0, nDir = 0, clearNx = 1, clearShift = 0;
};

// Is every table there that a launch of the problem needs?  The text of the refusal, or null.
inline const char *incomplete(const ProblemFacts &f) {
  for (const CompTables &t : f.comp)
    if (!t.inv) return "computeRadiativeTransfer: problem not completely specified (inverse phase function table missing).";
  for (const CompTables &t : f.comp)
    if (f.nDir > 0 && !t.fwd) return "computeRadiativeTransfer: problem not completely specified (forward phase function table missing).";
  return nullptr;
}

// The radiance path tally (EXTRA_RADIANCE_PATHS) is filled by the general radiance kernel of a plain, traced launch with at least one
// radiance direction: what the decision itself can see of that, as the text of the refusal behind the entry point's name, or null.
// (the directions' cosines and the contribution limit are the handle's: i3rc_hip.hip, extra_tally_refused)
inline const char *radiance_paths_refused(const ProblemFacts &f, const StreamKind &s) {
  if (f.extra != EXTRA_RADIANCE_PATHS && s.extra != EXTRA_RADIANCE_PATHS) return nullptr;
  if (s.batched)
    return "radiance path lengths have no batch statistics yet and are tallied by plain launches only; fused or announced batches cannot give them "
           "(switch them off, or call i3rc_hip_launch_batch per batch)";
  if (s.replay) return "radiance path lengths are tallied by plain launches only; the replay stream cannot give them (switch them off)";
  if (f.nDir < 1) return "radiance path lengths are tallied by radiance launches only; no radiance direction is set (nDir = 0)";
  if (!traced(f)) return "radiance path lengths need ray tracing; max cross-section is in use (useRayTracing = 0)";
  return nullptr;
}

// Dynamic LDS of one launch: the end of the kernel's own carve-up (lds_plan, tracer.hpp -- the function photon_kernel sets its
// pointers from), for the instantiation that is about to run.
inline size_t lds_bytes(const LaunchDecision &d, const StreamKind &s, bool direct, int nInv, bool tableInLds, bool startStore) {
  const bool intensity = d.nDir > 0;
  const LdsPlan lp = lds_plan(d, intensity && !s.replay, direct, d.place, intensity, tableInLds ? 16 : 4, tableInLds ? nInv : 0, startStore);
  size_t words = (size_t)lp.end;
  if (s.extra == EXTRA_TRACKS)   // the track-length sums behind the plan's end (photon_kernel, TRACK)
    if (d.ldsGrid & kLdsGridTrackSums) words = (size_t)track_sums_word(lp.end) + 2 * (size_t)d.nx * d.ny * d.nz;
  if (s.extra == EXTRA_PATH_BINS && d.ldsBins)   // the histogram's sums and edges, in the same place (photon_kernel, BINS)
    words = (size_t)track_sums_word(lp.end) + (size_t)bin_region_words(d.pathBins);
  return (sizeof(float) * words + 15) & ~(size_t)15;
}

// Everything the host decides about a launch of `kind` on the problem `f`.
inline LaunchDecision plan_launch(const ProblemFacts &f, const EnvKnobs &env, const LaunchKind &kind) {
  LaunchDecision d;
  const StreamKind &s = kind.stream;
  const bool fused = s.batched, replay = s.replay;
  const auto refuse = [&d](const char *text, bool early) { d.refusal = text; d.early = early; return d; };
  if (const char *missing = incomplete(f)) return refuse(missing, true);
  if (const char *paths = radiance_paths_refused(f, s)) return refuse((std::string("plan_launch: ") + paths).c_str(), true);
  d.nx = f.nx; d.ny = f.ny; d.nz = f.nz; d.ncomp = f.ncomp; d.nDir = f.nDir; d.clearNx = f.clearNx; d.clearShift = f.clearShift;
  // bricks pay off once the field no longer fits in one XCD's 4 MB of L2
  // (the clear-air map of a bricked field holds layer numbers in 16 bits: domains of more layers than that keep the linear field)
  // Column records where the field has them (and does not fit in LDS, below): the whole field in 8 bytes per column.  Measured:
  // I3RC_COLUMNS=0 switches them off for the process.
  // (records over a base profile -- GRID_COLBASE -- are read by the kernels of domains with several components, the general and the
  // several-components ones: the one-component specialisations and the replay build are not instantiated for them)
  const bool baseOk = f.ncomp > 1 && !replay;
  bool columns = (f.gridPlace == I3RC_GRID_COLUMNS || (f.gridPlace == I3RC_GRID_AUTO && env.columns && f.colRecords)) && (!f.colBase || baseOk);
  const bool bricksBeyondL2 = ncell_bytes(f) > ((size_t)4 << 20) && f.nz <= 65534;
  bool bricks = f.gridPlace == I3RC_GRID_BRICKS || (f.gridPlace == I3RC_GRID_AUTO && !columns && bricksBeyondL2);
  if (f.params.useSurfaceBDRF && !uniform_surface(f) && !f.surfaceSet)
    return refuse("computeRadiativeTransfer: surfaceBDRF requested but no surface description set", true);
  {
    i3rc_tally_layout layout; TallyView view;
    (void)tally_layout(f.nx, f.ny, f.nz, f.ncomp, f.nDir, f.extra, layout, view, f.pathBins);
    if (layout.total >= ((int64_t)1 << 31)) return refuse("tally buffer too large (2^31 elements or more)", true);
  }
  const size_t ncol = (size_t)f.nx * f.ny, ncell = ncol * f.nz;
  // (the radiance path tally's kernel has no one-direction form: it makes no ready rays at all, and keeps the ring kernels' carve-up)
  const bool direct = direct_rays(f, env) && s.extra != EXTRA_RADIANCE_PATHS;
  LdsEstimate lds{sizeof(float) * ((f.nx + 1) + (f.ny + 1) + (f.nz + 1) + 3 * (size_t)f.nDir)};
  // radiance runs: every wave's ring of local-estimate events (one record serves the nDir rays of an event) and its
  // buffer of ready-made rays (photon_kernel, ray mode)
  // (one direction: no ring, a ready store of two wavefronts -- photon_kernel, DIRECT)
  d.rayQueueCap = f.nDir > 0 && !direct ? 64 : 0;   // (an event phase pushes at most 64 records; the rays go on to the ready buffer)
  if (f.nDir > 0) lds.bytes += sizeof(float) * 4 * (kRecWords * (size_t)d.rayQueueCap + kReadyWords * (size_t)(direct ? kDirectReady : kReadyRays));
  if (f.nDir > 0) lds.bytes += sizeof(float) * (16 * (size_t)f.nDir + 3);   // per direction: what a ray derives from it (Lds::dirTab, 16-byte aligned)
  if (f.nDir > 0)
    for (int c = 0; c < f.ncomp; ++c)
      if (f.maxPfIndex[c] >= 65536) return refuse("radiance runs take at most 65535 phase-function table entries per component", true);
  if (!lds.fits(0, kLdsHard)) return refuse("domain edge vectors do not fit in LDS (nx + ny + nz beyond about 39 000)", true);
  // (records over a base profile keep the profile in LDS as well: where edges and profile together are beyond what a launch may
  // have, the automatic place reads the field as it would without the records -- in bricks beyond 4 MB, else linearly -- instead of
  // planning a launch that launch's own check refuses)
  bool base = columns && f.colBase;
  if (base && f.gridPlace == I3RC_GRID_AUTO && !lds.fits(sizeof(float) * (size_t)f.nz, kLdsHard)) {
    columns = base = false;
    if (bricksBeyondL2) bricks = true;
  }
  // (a fused multi-batch launch tallies per batch, straight into global memory: no partial sums in LDS)
  // (float64 partial sums: tracer.hpp, tally_t; + 4: their 8-byte alignment.  I3RC_LDS_TALLIES=0 / i3rc_hip_set_lds_tallies(h, 0): every
  // tally straight to the float64 buffer in global memory -- a measurement knob, and one more order of the same float64 additions)
  const bool privatise = !fused && env.ldsTallies && f.ldsTalliesOn;
  d.ldsTallies = privatise && lds.take(2 * ncol * sizeof(tally_t) + 4, kLdsBudget / 2);
  // (an absorbing domain of few cells -- the step cloud's 512 or 1024 --: its volume-absorption tallies, which every scattering adds to)
  d.ldsVolume = privatise && f.absorbing && lds.take(ncell * sizeof(tally_t) + 4, kLdsBudget / 2);
  {
    const size_t nInt = (size_t)(f.ncomp + 1) * f.nDir * ncol * sizeof(tally_t) + 4;
    d.ldsIntensity = privatise && f.nDir > 0 && nInt <= 16 * 1024 && lds.take(nInt, kLdsBudget);
  }
  if (f.gridPlace == I3RC_GRID_AUTO && lds.take(ncell * sizeof(float), kLdsBudget)) { d.ldsGrid = 1; columns = base = bricks = false; }   // (never when the edges alone are beyond the budget)
  else if (bricks && !columns && f.nDir == 0) lds.bytes += sizeof(uint32_t) * (size_t)f.clearWords;   // bricked field, flux kernels: its clear-air map
  if (base) lds.bytes += sizeof(float) * (size_t)f.nz;                                                 // column records over a base profile: the profile
  d.estimate = (lds.bytes + 15) & ~(size_t)15;
  const bool intensity = f.nDir > 0;
  const int place = d.place = d.ldsGrid ? GRID_LDS : (columns ? (base ? GRID_COLBASE : GRID_COLUMNS) : (bricks ? GRID_BRICKS : GRID_GLOBAL));
  const int nInv = f.comp[0].nInv;
  // The track-length sums (photon_kernel, TRACK): where the field itself lies in LDS, partial sums in LDS are switched on
  // (i3rc_hip_set_lds_tallies, I3RC_LDS_TALLIES) and the launch's allocation has room for one more float64 word per cell behind the
  // plan's end, the workgroups keep their track-length sums there: bit 1 of ldsGrid tells the kernel, the last plan says so.
  if (s.extra == EXTRA_TRACKS && place == GRID_LDS && env.ldsTallies && f.ldsTalliesOn) {
    d.ldsGrid |= kLdsGridTrackSums;
    if (lds_bytes(d, s, direct, nInv, false, false) > kLdsLaunchMax) d.ldsGrid &= ~kLdsGridTrackSums;
  }
  // The path histogram (photon_kernel, BINS): at ANY place of the field, where partial sums in LDS are switched on and the launch's
  // allocation with the region -- 4 (nBins + 1) float64 sums and the nBins + 1 edges behind the plan's end -- stays within the budget of a
  // workgroup, the workgroups keep their sums there; else the launch adds to the block in global memory.  Never a refusal.
  if (s.extra == EXTRA_PATH_BINS) {
    d.pathBins = f.pathBins;
    d.ldsBins = env.ldsTallies && f.ldsTalliesOn && f.pathBins >= 1;
    if (d.ldsBins && lds_bytes(d, s, direct, nInv, false, false) > kLdsBudget) d.ldsBins = 0;
  }
  // Which kernel runs the launch (see photon_kernel).  Fused launches (PhiloxBatchStream) are made for the specialised problems only
  // (fuse_loop): the common class, or the widened one.  Plain launches run the specialised kernels when the problem is in the common
  // class, the widened radiance kernels for radiance problems of the widened class, else the general kernel.
  KernelKey key{intensity, true, place, false, false, false};
  int threads = 256;
  // (an extra tally block: the general flux kernel whatever the problem's class, the radiance path tally's the general radiance kernel --
  // the key as it stands)
  if (!replay && s.extra == EXTRA_NONE) {   // (the replay build always runs the general kernel: it keeps the nested local estimate, no queue at all)
    bool simple, wide;
    if (fused) {
      // the widened class (several components, irregular x / y, a gridded surface): its own fused kernels, flux ones too -- a driver's
      // loop of 1e6-photon batches on Landsat-36 + gas then costs 1.1 ms per batch instead of 2.6 (profiles/r05_fused_wide.txt)
      simple = common_class(f, kind.srcKind);
      wide = !simple;
    } else {
      simple = common_class(f, kind.srcKind) && f.kernelVariant != I3RC_KERNEL_GENERAL && !(kNestedBuild && intensity);
      // several components, otherwise the common class: RADIANCE problems run photon_kernel<..., MULTI> (+20 % on the Landsat scene + gas
      // with seven directions against the general radiance kernels' 166 registers and three waves per SIMD).  Flux problems stay with
      // the general flux kernel: its several-components specialisation was built and measured -- 5.78 against 5.71e8 photons/s on
      // Landsat-119 + gas, 9.13 against 9.08e8 on Landsat-36 + gas: the voxel steps are the same code, and a flux event's few extra
      // reads do not show (profiles/r05_ab_experiments.txt) -- and is not in the tree.
      wide = !simple && intensity && multi_class(f, kind.srcKind) && f.kernelVariant != I3RC_KERNEL_GENERAL && !kNestedBuild;
    }
    key.general = !simple && !wide;
    key.wide = wide;
    key.direct = intensity && direct;
    // Flux problems of the common class with ONE phase-function entry keep the inverse table's cosines (40 KB) in LDS, in
    // workgroups of 1024 threads, two per compute unit (photon_kernel, TBL): the two dependent table reads of a scattering come
    // from LDS instead of L2 -- or, where the extinction field fills the L2 (Landsat-36: 2.4 MB of 4), instead of the fabric.
    // Step cloud 29.75 -> 29.29 ms per 1e8 photons (+1.6 %), radar 640 +2 %, Landsat-36 87.0 -> 71.0 ms (+22 %).  The fused
    // instantiations are planned for eight waves per SIMD -- two workgroups per compute unit -- and pay for it with two vector
    // registers in scratch.  I3RC_TABLE_LDS=0 switches both off.
    const bool placeOk = fused ? ((env.fusedPlaces >> place) & 1) && place != GRID_BRICKS
                               : ((env.plainPlaces >> place) & 1) && place != GRID_COLBASE && f.kernelVariant == I3RC_KERNEL_AUTO;
    // (the 16 waves' start stores -- photon_kernel, STORE: 16 KB -- count: two workgroups of 1024 threads share a compute unit's 160 KB.
    // A domain that had room for the table without them runs the 256-thread kernel of its place, as the domains just beyond it always did.)
    const size_t tblStore = s.startStore(intensity, false, place, false) ? start_store_bytes(1024) : 0;
    if (env.tableLds && simple && !intensity && placeOk && (f.uniformPf >= 1 || f.nInvEntries[0] == 1) &&
        LdsEstimate{d.estimate}.fits(sizeof(float) * (size_t)nInv + tblStore, kLdsTableForm)) {
      key.tbl = true;
      threads = 1024;
    }
  }
  // The start store comes on top of what has been placed in LDS above -- edges, tallies, the field: every domain keeps its place --
  // and is part of the launch's allocation (lds_bytes).  Where that would go beyond a compute unit's LDS (edge vectors of some 154 KB or
  // more: a column of 39 000 layers) the launch runs the general flux kernel, which has no store, instead of being refused.
  bool startStore = s.startStore(key.intensity, key.general, key.place, key.wide);
  if (startStore && lds_bytes(d, s, direct, nInv, key.tbl, true) > kLdsLaunchMax) {
    key.general = true; key.tbl = false; threads = 256;
    startStore = false;
  }
  d.key = key; d.threads = threads; d.startStore = startStore;
  d.startStoreBytes = startStore ? start_store_bytes(threads) : 0;
  d.ldsBytes = lds_bytes(d, s, direct, nInv, key.tbl, startStore);
  if (d.ldsBytes > kLdsLaunchMax) return refuse("the launch needs more LDS than a compute unit has", false);
  return d;
}

// what i3rc_hip_last_plan reports of a launch (binding.PLAN_NAMES); the chunk -- word kPlanChunk -- is known once the grid is (launch_grid)
constexpr int kPlanWords = 13, kPlanChunk = 11;
// (a fourteenth word, for callers that ask for it: the path histogram's sums in LDS -- binding.PLAN_BIN_NAME; it follows the thirteen in
// i3rc_hip_last_plan and the three of PLAN_EXTRA_NAMES in i3rc_hip_plan_launch, so that no earlier word moves)
constexpr int kPlanBinWord = kPlanWords;
constexpr int kFactWords = 23;   // the words of i3rc_hip_problem_facts (binding.FACT_NAMES)
inline void plan_words(const ProblemFacts &f, const LaunchDecision &d, int fusedBatches, int32_t *v) {
  const int32_t w[kPlanWords] = {d.ldsGrid ? 1 : 0, d.ldsTallies, d.ldsVolume, d.ldsIntensity, d.key.tbl ? 1 : 0, (int32_t)d.ldsBytes, f.absorbing ? 1 : 0,
                                 f.cellRecBytes, fusedBatches, d.place, (int32_t)d.startStoreBytes, 0, (d.ldsGrid & kLdsGridTrackSums) ? 1 : 0};
  std::memcpy(v, w, sizeof(w));
}

}  // namespace i3rc

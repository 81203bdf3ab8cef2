// C ABI (include/i3rc_hip.h) of the gfx950 photon-tracing integrator: device-state ownership, launches, tallies.
#include "../../include/i3rc_hip.h"

#include <hip/hip_runtime.h>
#include <ctime>
#include <map>
#include <utility>

#include "kernels.hpp"
#include "tally_block.hpp"
#include "launch_plan.hpp"

using namespace i3rc;

namespace {

thread_local std::string g_createError;

// I3RC_POISON=1 (debugging aid): fresh device memory is filled with 0xFF bytes -- NaNs as floats, -1 as integers, wild
// as pointers -- so that a read of memory nobody wrote shows in a fresh process and not only after other
// allocations have left their contents behind.
bool poison() { static const bool on = std::getenv("I3RC_POISON") != nullptr; return on; }

// I3RC_TRACE=1 (debugging aid): a line on stderr for every fused group launched, served late or called off
bool tracing() { static const bool on = std::getenv("I3RC_TRACE") != nullptr; return on; }
double trace_ms() {
  timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
  static const double t0 = ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6 - t0;
}


struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t upload(const void *src, size_t n) {
    hipError_t e = alloc(n);
    if (e != hipSuccess) return e;
    if (n) e = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    return e;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; } bytes = 0; }
  hipError_t alloc(size_t n) {
    if (p) { (void)hipFree(p); p = nullptr; }
    bytes = n;
    hipError_t e = hipMalloc(&p, n ? n : 4);
    if (e == hipSuccess && poison()) {
      // (hipMemset returns before the fill has happened, and the null stream does not order it against the library's
      // non-blocking streams: without the wait the poison lands on what the first kernels on those streams have written)
      e = hipMemset(p, 0xFF, n ? n : 4);
      if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return e;
  }
};

}  // namespace

struct i3rc_hip_integrator : ProblemFacts {   // (the facts every launch is decided from: launch_plan.hpp)
  int device = 0;
  std::vector<float> xE, yE, zE;  // host copies (launch parameters, checks)
  std::vector<double> areaFrac, layerDepth;   // what the normalisation needs of the grid (TallyView::areaFrac, ::dz), worked out once
  DevBuf dxE, dyE, dzE, dExt, dCum, dSsa, dPf;
  DevBuf dCellRec;               // two components: a scattering's reads of its cell as one 16-byte record (DevProblem::cellRec)
  DevBuf dExtBrick;              // totalExt in bricks of 32 cells (DevProblem::extBrick)
  DevBuf dClearMap;              // ... and its clear-air map (DevProblem::clearMap)
  DevBuf dColRec;                // one record per column where every column is one run of one value (DevProblem::colRec); else empty
  DevBuf dColBase;               // ... over a base profile (DevProblem::colBase, nz floats): the records then hold what lies ON the profile
  bool compDirty = true;         // comp[] changed since its device copy (dComp) was made
  std::vector<DevBuf> dInv, dInvCos, dFwd, dFwdOrig;   // per component (sized by i3rc_hip_create)
  DevBuf dComp;
  DevBuf dXs, dYs, dBrdf;
  float brdf0 = 0.f;          // reflectance of the first surface cell (a 1 x 1 surface grid is a plain Lambertian albedo)
  DevBuf dDir;
  std::vector<float> dirHost;   // the directions as set (the radiance path tally refuses a launch with a direction that does not point upwards)
  // the first flight of a zenith sun (first_flight.hpp): the column table, made at the first launch that could use it (first_flight)
  DevBuf dFlight;                // table[ny * nx][nz + 1]: the optical path after k downward steps from the start height
  int flightState = 0;           // 0: not made yet, 1: made and fit, 2: no table (its sweep met what makes it unfit, or it is too large)
  int flightLayer = 0;           // the start layer its kernel found (the photon kernels' izStart)
  bool flightOn = true;          // i3rc_hip_set_first_flight_table
  bool lastLanded = false;       // the most recent launch landed its photons from the table (i3rc_hip_last_first_flight)
  DevBuf dBins;                  // the path histogram's table as the kernels read it (BinTable, kernels.hpp): nBins, then the nBins + 1 edges
  std::vector<float> binEdges;   // ... and the edges' host copy (empty while the histogram is off)

  i3rc_tally_layout layout{};
  TallyView view{};                // the same block as the normalisation sees it (tally_block.hpp, tally_layout), over the host arrays above
  DevBuf ownTally;
  double *tally = nullptr;  // device pointer in use (own or bound)
  DevBuf workCounter;
  DevBuf srcBuf[5];

  // i3rc_hip_run_batches: batches in flight, each with a stream, a tally buffer, a work counter and a pinned host copy of its own
  struct PipeSlot {
    hipStream_t stream = nullptr;
    DevBuf tally, counter, excess;   // (excess: see accumulate_moments)
    double *pinned = nullptr;
    hipEvent_t done = nullptr;
    int batch = -1;            // batch whose tallies are on their way into `pinned`
  };
  static constexpr int kMaxInFlight = 8;
  PipeSlot pipe[kMaxInFlight];
  int64_t pipeTotal = 0;       // layout.total the slots were sized for
  // i3rc_hip_compute_batch: batches launched ahead of the caller's loop (oldest first, in slots of the same pool), all
  // with the signature below
  struct Ahead { uint32_t seed1; int slot; };
  std::vector<Ahead> aheadQueue;
  struct BatchSignature {
    uint32_t seed0 = 0; int64_t n = 0; float mu = 0.f, az = 0.f; bool set = false;
    bool operator==(const BatchSignature &o) const { return set && o.set && seed0 == o.seed0 && n == o.n && mu == o.mu && az == o.az; }
  } aheadSig, lastSig;
  uint32_t lastSeed1 = 0;

  // Fused multi-batch launches (i3rc_hip_run_batches / the look-ahead of i3rc_hip_compute_batch on problems the
  // specialised flux kernels run): a GROUP of consecutive batches is ONE grid (photon_kernel<PhiloxBatchStream, ...>), every
  // batch with tally blocks of its own -- `replicas` of them, summed by reduce_replicas_kernel into `compact` --, so that
  // one batch's tail is filled by the next batch's photons inside the launch.  Up to kFusedSlots groups are in flight, each
  // on a stream of its own (the tail of a group is covered by the next group; its copy to the host by the one after).
  struct FusedSlot {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t traced = nullptr;   // the group's blocks are complete on the device (its copy to the host waits for this on the copy stream)
    DevBuf blocks, compact, counter, counterBlocks, excess;
    double *pinned = nullptr; size_t pinnedBytes = 0;
    int *abortFlag = nullptr;      // host-coherent word the kernel polls (RunArgs::abortFlag)
    int first = 0, count = 0;      // batches first .. first + count - 1 of the call (count = 0: free)
    uint32_t seed1 = 0;            // seed word of the group's first batch
    int next = 0;                  // look-ahead: batches of the group handed to the caller so far
  };
  static constexpr int kFusedSlots = 3;
  FusedSlot fused[kFusedSlots];
  // The groups' copies to the host go over a stream of their own: a copy engine does not take compute units from the next group's
  // kernel (kernels of two streams are time-sliced against each other, which is why the groups themselves share one stream), and
  // a Landsat-sized group is 100-250 MB -- 4-10 ms of PCIe during which the next group's kernel used to wait in the queue.
  hipStream_t fusedCopyStream = nullptr;
  std::vector<int> aheadGroups;    // look-ahead: slots of the groups launched ahead, oldest first
  int aheadGroupSize = 0;          // size of the next group to launch ahead (grows 8, 16, 32 ... 256)
  bool aheadBounded = false;       // i3rc_hip_expect_batches: the caller has announced its loop -- nothing is launched beyond
  uint32_t aheadEnd = 0;           // ... this seed word (exclusive)
  int fusion = -1;                 // -1: automatic, 0: never fuse, 1: fuse whatever the batch size (i3rc_hip_set_batch_fusion)
  bool fusedAheadFailed = false;   // a fused group could not be launched ahead (memory): look ahead with single batches until the layout changes
  // i3rc_hip_run_batches_moments: sums and sums of squares over a loop's batches, accumulated on the device (momArea / momDz: the
  // device copies of areaFrac / layerDepth)
  DevBuf momSum, momSq, momCounters, momArea, momDz;
  // i3rc_hip_run_batches_diagnostic_moments: the same of the optional diagnostic tally (extra_moments_layout), sized by the kind
  DevBuf momExtraSum, momExtraSq;
  // i3rc_hip_run_batches_path_moments: the same of the two path tallies (path_moments_layout), and the absorption coefficients of the
  // spectrum (i3rc_hip_set_path_spectrum) with their device copy
  DevBuf momPathSum, momPathSq, dPathK;
  std::vector<float> pathK;

  // XCD-aware photon order (launch): the sorted photon numbers and the slab bookkeeping of a launch, per stream (launches
  // on different streams -- i3rc_hip_run_batches -- are in flight together)
  struct SlabBufs { DevBuf ids, meta, blockCounts, blockBase; };
  std::map<hipStream_t, SlabBufs> slabBufs;

  hipStream_t ownStream = nullptr, stream = nullptr;
  static constexpr int kEventRing = 64;   // HIP-event pairs of the most recent timed launches
  hipEvent_t evStart[kEventRing] = {}, evStop[kEventRing] = {};
  long long timedLaunches = 0;
  int numCU = 256;
  int evThreshold = 0;        // lanes waiting before a wave runs its event phase; 0 = adapted per wave
  int lightThreshold = 0;     // lanes with an ended shadow ray before a wave runs its light phase; 0 = adapted per wave
  int blocksPerCU = 0;  // 0 = from occupancy query
  std::string lastKernelName;            // kernel the most recent launch ran (i3rc_hip_last_kernel_name)
  int32_t lastPlan[kPlanWords] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // ... and its plan (i3rc_hip_last_plan)
  int32_t lastPlanBins = -1;             // ... and that plan's fourteenth word (kPlanBinWord)
  int64_t launchLimit = 0;               // photons per kernel launch (i3rc_hip_set_launch_limit); 0 = numCU * 2^22
  std::string err;

  int fail(const std::string &m) { err = m; return 1; }
  int hipfail(const char *what, hipError_t e) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    return 1;
  }
};

#define HIPCHK(h, call)                                   \
  do {                                                    \
    hipError_t e__ = (call);                              \
    if (e__ != hipSuccess) return (h)->hipfail(#call, e__); \
  } while (0)

static void compute_layout(i3rc_hip_integrator *h) {
  TallyView &V = h->view;
  (void)tally_layout(h->nx, h->ny, h->nz, h->ncomp, h->nDir, h->extra, h->layout, V, h->pathBins);
  V.xyRegular = h->xyRegular;
  V.areaFrac = h->areaFrac.data(); V.dz = h->layerDepth.data();
}
// where the actinic flux's track-length sums lie in the packed buffer, -1 while they are off
static int64_t track_block(const i3rc_hip_integrator *h) { return h->extra == EXTRA_TRACKS ? extra_block_offset(h->layout.counters) : -1; }

// The handle's view as a call finds it: whether limited contributions are redistributed is a parameter (i3rc_hip_set_params), which
// changes without the layout.
static TallyView current_view(const i3rc_hip_integrator *h) {
  TallyView V = h->view;
  V.limitContrib = h->nDir > 0 && h->params.limitIntensityContributions;
  return V;
}

static int realloc_tally(i3rc_hip_integrator *h) {
  compute_layout(h);
  HIPCHK(h, h->ownTally.alloc((size_t)h->layout.total * sizeof(double)));
  HIPCHK(h, hipMemset(h->ownTally.p, 0, (size_t)h->layout.total * sizeof(double)));
  h->tally = (double *)h->ownTally.p;
  return 0;
}

// Batches launched ahead by i3rc_hip_compute_batch read the handle's device arrays: whatever changes those (tables,
// parameters, surface, directions, tuning) waits for them first and forgets them.
static void drop_lookahead(i3rc_hip_integrator *h) {
  if (tracing() && (!h->aheadGroups.empty() || !h->aheadQueue.empty()))
    std::fprintf(stderr, "[i3rc %9.3f ms] look-ahead called off (%d fused groups, %d single batches)\n", trace_ms(), (int)h->aheadGroups.size(), (int)h->aheadQueue.size());
  for (const int k : h->aheadGroups) {   // fused groups launched ahead: called off (their waves take no further chunks), then awaited
    auto &g = h->fused[k];
    if (g.abortFlag) __atomic_store_n(g.abortFlag, 1, __ATOMIC_RELEASE);
  }
  for (const int k : h->aheadGroups) {
    auto &g = h->fused[k];
    (void)hipStreamSynchronize(g.stream);
    g.count = 0;
  }
  if (!h->aheadGroups.empty() && h->fusedCopyStream) (void)hipStreamSynchronize(h->fusedCopyStream);
  h->aheadGroups.clear();
  h->aheadGroupSize = 0;
  h->aheadBounded = false;
  for (const auto &a : h->aheadQueue) {
    (void)hipStreamSynchronize(h->pipe[a.slot].stream);
    h->pipe[a.slot].batch = -1;
  }
  h->aheadQueue.clear();
  h->aheadSig.set = false; h->lastSig.set = false;
}

// The words in which the error texts speak of each kind of the optional diagnostic tally
struct ExtraWords { const char *setter, *noun, *are, *need, *them, *their, *possessive; };
static const ExtraWords kExtraWords[] = {
    {},
    {"i3rc_hip_set_level_fluxes", "level fluxes", "are", "need", "them", "their", "the level fluxes'"},
    {"i3rc_hip_set_actinic_flux", "the actinic flux", "is", "needs", "it", "its", "the actinic flux's"},
    {"i3rc_hip_set_path_lengths", "path lengths", "are", "need", "them", "their", "the path lengths'"},
    {"i3rc_hip_set_path_histogram", "the path histogram", "is", "needs", "it", "its", "the path histogram's"},
    {"i3rc_hip_set_radiance_path_lengths", "radiance path lengths", "are", "need", "them", "their", "the radiance path lengths'"}};

// Switches one kind of the optional diagnostic tally on or off (i3rc_hip_set_level_fluxes, i3rc_hip_set_actinic_flux, i3rc_hip_set_path_lengths,
// i3rc_hip_set_path_histogram -- whose block is sized by nBins: switching it on while it is on lays the block out anew, cleared).
static int set_extra_tally(i3rc_hip_integrator *h, ExtraTally kind, bool on, int nBins = 0) {
  if (!h) return 1;
  drop_lookahead(h);
  if ((h->extra == kind) == on && !(on && kind == EXTRA_PATH_BINS)) return 0;
  const ExtraWords &w = kExtraWords[kind];
  if (on && h->extra != EXTRA_NONE && h->extra != kind) {   // the other kind's block lies in the same place
    const ExtraWords &o = kExtraWords[h->extra];
    return h->fail(std::string(w.setter) + ": " + o.noun + " " + o.are + " switched on and " + o.their + " block lies where " + w.possessive +
                   " would; switch " + o.them + " off first (no kernel tallies both)");
  }
  // the tally layout changes: as for a change of nDir, a caller-bound buffer is refused before anything is touched
  if (h->tally != (double *)h->ownTally.p)
    return h->fail(std::string(w.setter) + ": a caller-bound tally buffer is in use; unbind it (bind NULL) before switching " + w.noun +
                   ", then bind a buffer of the new layout's size");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (launches in flight add to the buffer that is about to be replaced)
  h->extra = on ? kind : EXTRA_NONE;
  h->pathBins = on ? nBins : 0;
  return realloc_tally(h);
}

// The slots of i3rc_hip_run_batches / i3rc_hip_compute_batch are kept with the handle (streams and pinned memory are
// expensive to make); a new tally layout invalidates their buffers.
static int reset_slots_if_layout_changed(i3rc_hip_integrator *h) {
  if (h->pipeTotal == h->layout.total) return 0;
  drop_lookahead(h);
  for (auto &sl : h->pipe) {
    if (sl.stream) HIPCHK(h, hipStreamSynchronize(sl.stream));
    if (sl.pinned) { HIPCHK(h, hipHostFree(sl.pinned)); sl.pinned = nullptr; }
    sl.batch = -1;
  }
  h->pipeTotal = h->layout.total;
  h->fusedAheadFailed = false;
  return 0;
}
static int ready_slot(i3rc_hip_integrator *h, int k) {
  auto &sl = h->pipe[k];
  const size_t bytes = (size_t)h->layout.total * sizeof(double);
  if (!sl.stream) HIPCHK(h, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
  if (!sl.done) HIPCHK(h, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
  if (!sl.counter.p) HIPCHK(h, sl.counter.alloc(sizeof(unsigned long long)));
  if (!sl.pinned) HIPCHK(h, hipHostMalloc((void **)&sl.pinned, bytes, hipHostMallocDefault));
  if (sl.tally.bytes != bytes) HIPCHK(h, sl.tally.alloc(bytes));
  return 0;
}

extern "C" {

const char *i3rc_hip_version(void) { return "i3rc_hip 0.1 (gfx950)"; }

int i3rc_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  return n;
}

const char *i3rc_hip_last_error(const i3rc_hip_integrator *h) { return h ? h->err.c_str() : g_createError.c_str(); }

int i3rc_hip_create(i3rc_hip_integrator **out, int device, int nx, int ny, int nz, int ncomp, const float *xEdges,
                    const float *yEdges, const float *zEdges, const float *totalExt, const float *cumExt, const float *ssa,
                    const int32_t *pfIndex) {
  if (!out) { g_createError = "i3rc_hip_create: null handle pointer"; return 1; }
  *out = nullptr;
  if (nx < 1 || ny < 1 || nz < 1 || ncomp < 1 || ncomp > I3RC_MAX_COMPONENTS) {
    g_createError = "i3rc_hip_create: bad dimensions (need nx,ny,nz >= 1 and 1 <= ncomp <= 255)";
    return 1;
  }
  if ((int64_t)nx * ny * nz > (int64_t)1 << 30 || (int64_t)nx * ny >= (int64_t)1 << 24 || nz >= 1 << 24) {
    g_createError = "i3rc_hip_create: domain too large (need nx*ny < 2^24, nx*ny*nz <= 2^30)";
    return 1;
  }
  if (!xEdges || !yEdges || !zEdges || !totalExt || !cumExt || !ssa || !pfIndex) {
    g_createError = "i3rc_hip_create: null array";
    return 1;
  }
  for (int i = 0; i < nx; ++i) if (!(xEdges[i + 1] > xEdges[i])) { g_createError = "i3rc_hip_create: x edges must increase"; return 1; }
  for (int i = 0; i < ny; ++i) if (!(yEdges[i + 1] > yEdges[i])) { g_createError = "i3rc_hip_create: y edges must increase"; return 1; }
  for (int i = 0; i < nz; ++i) if (!(zEdges[i + 1] > zEdges[i])) { g_createError = "i3rc_hip_create: z edges must increase"; return 1; }
  // the facts of the field, from the host arrays alone and before anything touches the device (launch_plan.hpp)
  auto *h = new i3rc_hip_integrator();
  ColumnRecords cols;
  g_createError = derive_facts(*h, EnvKnobs::process(), nx, ny, nz, ncomp, xEdges, yEdges, zEdges, totalExt, cumExt, ssa, pfIndex, &cols);
  if (!g_createError.empty()) { delete h; return 1; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1) {
    g_createError = "i3rc_hip_create: no HIP device available (the integrator has no CPU fallback)";
    delete h;
    return 2;
  }
  if (device < 0 || device >= ndev) { g_createError = "i3rc_hip_create: device index out of range"; delete h; return 1; }
  h->device = device;
  h->dInv = std::vector<DevBuf>(ncomp); h->dInvCos = std::vector<DevBuf>(ncomp); h->dFwd = std::vector<DevBuf>(ncomp); h->dFwdOrig = std::vector<DevBuf>(ncomp);
  auto bail = [&](const char *what, hipError_t er) {
    g_createError = std::string(what) + ": " + hipGetErrorString(er);
    delete h;
    return 1;
  };
#define CCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return bail(#call, e_); } while (0)
  CCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  CCHK(hipGetDeviceProperties(&prop, device));
  h->numCU = prop.multiProcessorCount;
  h->xE.assign(xEdges, xEdges + nx + 1);
  h->yE.assign(yEdges, yEdges + ny + 1);
  h->zE.assign(zEdges, zEdges + nz + 1);
  h->layerDepth.resize((size_t)nz); h->areaFrac.resize((size_t)nx * ny);
  grid_fractions(nx, ny, nz, xEdges, yEdges, zEdges, h->areaFrac.data(), h->layerDepth.data());
  const size_t ncell = (size_t)nx * ny * nz;
  CCHK(h->dxE.upload(xEdges, sizeof(float) * (nx + 1)));
  CCHK(h->dyE.upload(yEdges, sizeof(float) * (ny + 1)));
  CCHK(h->dzE.upload(zEdges, sizeof(float) * (nz + 1)));
  {
    // one layer of zeros on top: the tracer asks for the extinction of its cell before it looks at the step, and a
    // photon that starts within spacing() of the domain top has zIndex nz + 1 (it is dropped by that very step)
    std::vector<float> padded(ncell + (size_t)nx * ny, 0.0f);
    std::copy(totalExt, totalExt + ncell, padded.begin());
    CCHK(h->dExt.upload(padded.data(), sizeof(float) * padded.size()));
  }
  {
    std::vector<float> brick((size_t)h->nbx * h->nby * h->nbz * 32, 0.0f);
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
          const size_t b = ((size_t)(k >> h->bsz) * h->nby + (size_t)(j >> h->bsy)) * h->nbx + (size_t)(i >> h->bsx);
          const size_t w = ((size_t)(k & ((1 << h->bsz) - 1)) << (h->bsx + h->bsy)) | ((size_t)(j & ((1 << h->bsy) - 1)) << h->bsx) |
                           (size_t)(i & ((1 << h->bsx) - 1));
          brick[b * 32 + w] = totalExt[((size_t)k * ny + j) * nx + i];
        }
    CCHK(h->dExtBrick.upload(brick.data(), sizeof(float) * brick.size()));
    const int sft = h->clearShift;
    std::vector<uint32_t> lo((size_t)h->clearWords, 0xffffu), hi((size_t)h->clearWords, 0u), map((size_t)h->clearWords);
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i)
          if (totalExt[((size_t)k * ny + j) * nx + i] != 0.0f) {   // (NaN or negative values count as "something there": they are read as before)
            const size_t c = (size_t)(j >> sft) * h->clearNx + (size_t)(i >> sft);
            lo[c] = std::min<uint32_t>(lo[c], (uint32_t)std::min(k + 1, 0xfffe));
            hi[c] = std::max<uint32_t>(hi[c], (uint32_t)std::min(k + 1, 0xffff));
          }
    for (size_t c = 0; c < map.size(); ++c) map[c] = lo[c] | (hi[c] << 16);
    CCHK(h->dClearMap.upload(map.data(), sizeof(uint32_t) * map.size()));
  }
  if (h->colRecords) CCHK(h->dColRec.upload(cols.rec.data(), sizeof(uint32_t) * cols.rec.size()));
  if (h->colBase) CCHK(h->dColBase.upload(cols.base.data(), sizeof(float) * cols.base.size()));
  CCHK(h->dCum.upload(cumExt, sizeof(float) * ncell * ncomp));
  CCHK(h->dSsa.upload(ssa, sizeof(float) * ncell * ncomp));
  CCHK(h->dPf.upload(pfIndex, sizeof(int32_t) * ncell * ncomp));
  if (h->cellRecBytes == 8) {   // one component: {ssa, pfIndex}
    std::vector<uint32_t> rec(2 * ncell);
    for (size_t i = 0; i < ncell; ++i) { std::memcpy(&rec[2 * i], &ssa[i], 4); rec[2 * i + 1] = (uint32_t)pfIndex[i]; }
    if (h->dCellRec.upload(rec.data(), sizeof(uint32_t) * rec.size()) != hipSuccess) { g_createError = "i3rc_hip_create: device allocation of the cell records failed"; delete h; return 1; }
  } else if (h->cellRecBytes) {
    auto bits = [](float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; };
    const size_t words = ncomp == 2 ? 4 : 8;
    std::vector<uint32_t> rec(words * ncell, 0u);
    for (size_t i = 0; i < ncell; ++i) {
      uint32_t *r = &rec[words * i];
      const uint32_t pf01 = (uint32_t)pfIndex[i] | ((uint32_t)pfIndex[ncell + i] << 16);
      if (ncomp == 2) { r[0] = bits(cumExt[i]); r[1] = bits(ssa[i]); r[2] = bits(ssa[ncell + i]); r[3] = pf01; }
      else {
        r[0] = bits(cumExt[i]); r[1] = bits(cumExt[ncell + i]); r[2] = bits(ssa[i]); r[3] = bits(ssa[ncell + i]);
        r[4] = bits(ssa[2 * ncell + i]); r[5] = pf01; r[6] = (uint32_t)pfIndex[2 * ncell + i];
      }
    }
    CCHK(h->dCellRec.upload(rec.data(), sizeof(uint32_t) * rec.size()));
  }
  CCHK(h->workCounter.alloc(sizeof(unsigned long long)));
  CCHK(h->dComp.alloc(sizeof(CompTables) * ncomp));
  CCHK(h->dDir.alloc(sizeof(float) * 3 * I3RC_MAX_DIRECTIONS));
  CCHK(hipStreamCreateWithFlags(&h->ownStream, hipStreamNonBlocking));
  h->stream = h->ownStream;
  for (int i = 0; i < i3rc_hip_integrator::kEventRing; ++i) {
    CCHK(hipEventCreate(&h->evStart[i]));
    CCHK(hipEventCreate(&h->evStop[i]));
  }
#undef CCHK
  // defaults of type(integrator) :54-129
  h->params.surfaceAlbedo = 0.f; h->params.useSurfaceBDRF = 0; h->params.useRayTracing = 1; h->params.useRussianRoulette = 1;
  h->params.useHybridPhaseFunsForIntenCalcs = 0; h->params.numOrdersOrigPhaseFunIntenCalcs = 0;
  h->params.useRussianRouletteForIntensity = 0; h->params.zetaMin = 0.3f; h->params.limitIntensityContributions = 0;
  h->params.maxIntensityContribution = FLT_MAX;
  if (realloc_tally(h)) { g_createError = h->err; delete h; return 1; }
  *out = h;
  return 0;
}

int i3rc_hip_destroy(i3rc_hip_integrator *h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  // (first of all: whatever was launched ahead of the caller is called off -- destroying a stream waits for the device)
  for (auto &g : h->fused) if (g.abortFlag) __atomic_store_n(g.abortFlag, 1, __ATOMIC_RELEASE);
  if (tracing()) std::fprintf(stderr, "[i3rc %9.3f ms] destroy begins\n", trace_ms());
  for (auto &g : h->fused) if (g.stream && g.count > 0) { (void)hipStreamSynchronize(g.stream); break; }
  if (h->ownStream) { (void)hipStreamSynchronize(h->ownStream); (void)hipStreamDestroy(h->ownStream); }
  for (auto &sl : h->pipe) {
    if (sl.stream) { (void)hipStreamSynchronize(sl.stream); (void)hipStreamDestroy(sl.stream); }
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.pinned) (void)hipHostFree(sl.pinned);
  }
  for (auto &g : h->fused) if (g.abortFlag) __atomic_store_n(g.abortFlag, 1, __ATOMIC_RELEASE);
  if (tracing()) std::fprintf(stderr, "[i3rc %9.3f ms] destroy: abort words set\n", trace_ms());
  if (const hipStream_t s = h->fused[0].stream) {   // (the slots share the first one's stream)
    (void)hipStreamSynchronize(s);
    if (tracing()) std::fprintf(stderr, "[i3rc %9.3f ms] destroy: fused stream drained\n", trace_ms());
    (void)hipStreamDestroy(s);
  }
  for (auto &g : h->fused) {
    if (g.done) (void)hipEventDestroy(g.done);
    if (g.traced) (void)hipEventDestroy(g.traced);
    if (g.pinned) (void)hipHostFree(g.pinned);
    if (g.abortFlag) (void)hipHostFree(g.abortFlag);
  }
  if (h->fusedCopyStream) { (void)hipStreamSynchronize(h->fusedCopyStream); (void)hipStreamDestroy(h->fusedCopyStream); }
  for (int i = 0; i < i3rc_hip_integrator::kEventRing; ++i) {
    if (h->evStart[i]) (void)hipEventDestroy(h->evStart[i]);
    if (h->evStop[i]) (void)hipEventDestroy(h->evStop[i]);
  }
  delete h;
  return 0;
}

int i3rc_hip_set_inverse_table(i3rc_hip_integrator *h, int comp, int nSteps, int nEntries, const float *t) {
  if (!h) return 1;
  drop_lookahead(h);
  if (comp < 1 || comp > h->ncomp) return h->fail("i3rc_hip_set_inverse_table: component out of range");
  if (nSteps < 2 || nEntries < 1 || !t) return h->fail("i3rc_hip_set_inverse_table: bad table");
  if (nEntries < h->maxPfIndex[comp - 1]) return h->fail("i3rc_hip_set_inverse_table: phaseFunctionIndex refers to a missing table entry");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->dInv[comp - 1].upload(t, sizeof(float) * (size_t)nSteps * nEntries));
  // cos of every tabulated angle, in float64, rounded once (see scattering_cosine in tracer.hpp)
  std::vector<float> cosTab((size_t)nSteps * nEntries);
  for (size_t i = 0; i < cosTab.size(); ++i) cosTab[i] = (float)std::cos((double)t[i]);
  HIPCHK(h, h->dInvCos[comp - 1].upload(cosTab.data(), sizeof(float) * cosTab.size()));
  h->comp[comp - 1].inv = (const float *)h->dInv[comp - 1].p;
  h->comp[comp - 1].invCos = (const float *)h->dInvCos[comp - 1].p;
  h->comp[comp - 1].nInv = nSteps;
  h->compDirty = true;
  h->nInvEntries[comp - 1] = nEntries;
  return 0;
}

int i3rc_hip_set_forward_tables(i3rc_hip_integrator *h, int comp, int nSteps, int nEntries, const float *hybrid, const float *orig) {
  if (!h) return 1;
  drop_lookahead(h);
  if (comp < 1 || comp > h->ncomp) return h->fail("i3rc_hip_set_forward_tables: component out of range");
  if (nSteps < 2 || nEntries < 1 || !hybrid) return h->fail("i3rc_hip_set_forward_tables: bad table");
  if (nEntries < h->maxPfIndex[comp - 1]) return h->fail("i3rc_hip_set_forward_tables: phaseFunctionIndex refers to a missing table entry");
  if (!orig) orig = hybrid;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->dFwd[comp - 1].upload(hybrid, sizeof(float) * (size_t)nSteps * nEntries));
  HIPCHK(h, h->dFwdOrig[comp - 1].upload(orig, sizeof(float) * (size_t)nSteps * nEntries));
  h->comp[comp - 1].fwd = (const float *)h->dFwd[comp - 1].p;
  h->comp[comp - 1].fwdOrig = (const float *)h->dFwdOrig[comp - 1].p;
  h->comp[comp - 1].nFwd = nSteps;
  h->compDirty = true;
  h->nFwdEntries[comp - 1] = nEntries;
  return 0;
}

int i3rc_hip_set_params(i3rc_hip_integrator *h, const i3rc_params *p) {
  if (!h) return 1;
  drop_lookahead(h);
  if (!p) return h->fail("i3rc_hip_set_params: null params");
  if (!p->useSurfaceBDRF && (p->surfaceAlbedo > 1.f || p->surfaceAlbedo < 0.f))
    return h->fail("specifyParameters: surface albedo out of range.");  // :878-879
  if (p->useSurfaceBDRF && !h->surfaceSet) return h->fail("specifyParameters: surface description isn't valid.");  // :882-883
  if (p->zetaMin < 0.f) return h->fail("specifyParameters: zetaMin must be >= 0.");
  h->params = *p;
  return 0;
}

int i3rc_hip_set_surface(i3rc_hip_integrator *h, int nxs, int nys, const float *xs, const float *ys, const float *brdf) {
  if (!h) return 1;
  drop_lookahead(h);
  if (nxs < 1 || nys < 1 || !xs || !ys || !brdf) return h->fail("i3rc_hip_set_surface: bad surface grid");
  for (int i = 0; i < nxs; ++i) if (!(xs[i + 1] > xs[i])) return h->fail("new_SurfaceDescription: positions must be unique, increasing.");
  for (int i = 0; i < nys; ++i) if (!(ys[i + 1] > ys[i])) return h->fail("new_SurfaceDescription: positions must be unique, increasing.");
  for (size_t i = 0; i < (size_t)nxs * nys; ++i)
    if (brdf[i] < 0.f || brdf[i] > 1.f) return h->fail("new_SurfaceDescription: surface reflectance must be between 0 and 1");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, h->dXs.upload(xs, sizeof(float) * (nxs + 1)));
  HIPCHK(h, h->dYs.upload(ys, sizeof(float) * (nys + 1)));
  HIPCHK(h, h->dBrdf.upload(brdf, sizeof(float) * (size_t)nxs * nys));
  h->nxs = nxs; h->nys = nys; h->surfaceSet = true;
  h->brdf0 = brdf[0];
  return 0;
}

int i3rc_hip_set_directions(i3rc_hip_integrator *h, int nDir, const float *dirCos) {
  if (!h) return 1;
  drop_lookahead(h);
  if (nDir < 0 || nDir > I3RC_MAX_DIRECTIONS) return h->fail("i3rc_hip_set_directions: 0 <= nDir <= 255 required");
  if (nDir > 0 && !dirCos) return h->fail("i3rc_hip_set_directions: null directions");
  for (int d = 0; d < nDir; ++d)
    if (std::fabs(dirCos[3 * d + 2]) < FLT_MIN) return h->fail("specifyParameters: intensityMus can't be 0 (directly sideways)");  // :932-933
  // A change of nDir changes the tally layout.  With a caller-bound tally buffer that is refused BEFORE anything is
  // touched: nDir, the device copy of the directions and the layout all stay as they are (the caller unbinds --
  // i3rc_hip_bind_tally_buffer(h, NULL, 0) --, sets the directions, asks for the new layout and binds a buffer of that size).
  const bool changed = nDir != h->nDir;
  if (changed && h->tally != (double *)h->ownTally.p)
    return h->fail("i3rc_hip_set_directions: a caller-bound tally buffer is in use; unbind it (bind NULL) before changing nDir, "
                   "then bind a buffer of the new layout's size");
  HIPCHK(h, hipSetDevice(h->device));
  // launches in flight on the (possibly non-blocking) stream read dDir / the tally buffer: drain them first
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nDir > 0) HIPCHK(h, hipMemcpy(h->dDir.p, dirCos, sizeof(float) * 3 * nDir, hipMemcpyHostToDevice));
  h->nDir = nDir;
  h->dirHost.clear();
  if (nDir > 0) h->dirHost.assign(dirCos, dirCos + 3 * nDir);
  if (changed) return realloc_tally(h);   // (the radiance path block is sized by nDir: laid out anew with the radiance fields)
  return 0;
}

int i3rc_hip_get_tally_layout(const i3rc_hip_integrator *h, i3rc_tally_layout *layout) {
  if (!h || !layout) return 1;
  *layout = h->layout;
  return 0;
}

int i3rc_hip_bind_tally_buffer(i3rc_hip_integrator *h, void *devicePtr, size_t bytes) {
  if (!h) return 1;
  if (!devicePtr) { h->tally = (double *)h->ownTally.p; return 0; }
  if (bytes < (size_t)h->layout.total * sizeof(double)) return h->fail("i3rc_hip_bind_tally_buffer: buffer too small");
  if (((uintptr_t)devicePtr & 7u) != 0) return h->fail("i3rc_hip_bind_tally_buffer: buffer must be 8-byte aligned");
  h->tally = (double *)devicePtr;
  return 0;
}

int i3rc_hip_set_stream(i3rc_hip_integrator *h, void *s) {
  if (!h) return 1;
  h->stream = (hipStream_t)s;   // NULL is HIP's null stream (what torch.cuda.current_stream() is by default)
  return 0;
}

int i3rc_hip_use_own_stream(i3rc_hip_integrator *h) {
  if (!h) return 1;
  h->stream = h->ownStream;
  return 0;
}

int i3rc_hip_zero_tallies(i3rc_hip_integrator *h) {
  if (!h) return 1;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemsetAsync(h->tally, 0, (size_t)h->layout.total * sizeof(double), h->stream));
  return 0;
}

int i3rc_hip_set_level_fluxes(i3rc_hip_integrator *h, int on) { return set_extra_tally(h, EXTRA_LEVELS, on != 0); }

int i3rc_hip_get_level_flux_layout(const i3rc_hip_integrator *h, int64_t *up, int64_t *down, int64_t *total) {
  if (!h) return 1;
  if (up) *up = h->view.levelUp;
  if (down) *down = h->view.levelDown;
  if (total) *total = h->layout.total;
  return 0;
}

int i3rc_hip_set_actinic_flux(i3rc_hip_integrator *h, int on) { return set_extra_tally(h, EXTRA_TRACKS, on != 0); }

int i3rc_hip_get_actinic_flux_layout(const i3rc_hip_integrator *h, int64_t *offset, int64_t *total) {
  if (!h) return 1;
  if (offset) *offset = track_block(h);
  if (total) *total = h->layout.total;
  return 0;
}

int i3rc_hip_set_path_lengths(i3rc_hip_integrator *h, int on) { return set_extra_tally(h, EXTRA_PATHS, on != 0); }

int i3rc_hip_get_path_length_layout(const i3rc_hip_integrator *h, int64_t *up1, int64_t *up2, int64_t *down1, int64_t *down2, int64_t *total) {
  if (!h) return 1;
  if (up1) *up1 = h->view.pathUp1;
  if (up2) *up2 = h->view.pathUp2;
  if (down1) *down1 = h->view.pathDown1;
  if (down2) *down2 = h->view.pathDown2;
  if (total) *total = h->layout.total;
  return 0;
}

int i3rc_hip_set_radiance_path_lengths(i3rc_hip_integrator *h, int on) { return set_extra_tally(h, EXTRA_RADIANCE_PATHS, on != 0); }

int i3rc_hip_get_radiance_path_length_layout(const i3rc_hip_integrator *h, int64_t *path1, int64_t *path2, int64_t *total) {
  if (!h) return 1;
  if (path1) *path1 = h->view.radiancePath1;
  if (path2) *path2 = h->view.radiancePath2;
  if (total) *total = h->layout.total;
  return 0;
}

int i3rc_hip_set_path_histogram(i3rc_hip_integrator *h, int nBins, const float *edges) {
  if (!h) return 1;
  if (nBins == 0) {
    if (h->extra != EXTRA_PATH_BINS) { drop_lookahead(h); return 0; }
    if (set_extra_tally(h, EXTRA_PATH_BINS, false)) return 1;
    h->binEdges.clear();
    return 0;
  }
  // (bad bins are refused before anything is touched: a histogram that is on stays on, with the bins it had)
  const std::string who = "i3rc_hip_set_path_histogram: ";
  if (nBins < 0 || nBins > kMaxPathBins) return h->fail(who + "1 <= nBins <= " + std::to_string(kMaxPathBins) + " required (0 switches the histogram off); got " + std::to_string(nBins));
  if (!edges) return h->fail(who + "null edges (nBins + 1 float32 values)");
  for (int b = 0; b <= nBins; ++b)
    if (!std::isfinite(edges[b])) return h->fail(who + "edges must be finite; edges[" + std::to_string(b) + "] is not");
  if (edges[0] != 0.0f) return h->fail(who + "edges[0] must be 0 (a path length is never below it)");
  for (int b = 0; b < nBins; ++b)
    if (!(edges[b] < edges[b + 1]))
      return h->fail(who + "edges must be strictly ascending; edges[" + std::to_string(b + 1) + "] is not above edges[" + std::to_string(b) + "]");
  if (set_extra_tally(h, EXTRA_PATH_BINS, true, nBins)) return 1;
  h->binEdges.assign(edges, edges + nBins + 1);
  std::vector<float> table((size_t)nBins + 2);
  std::memcpy(&table[0], &nBins, sizeof(float));   // (word 0: nBins as an integer)
  std::copy(edges, edges + nBins + 1, table.begin() + 1);
  const hipError_t e = h->dBins.upload(table.data(), sizeof(float) * table.size());
  if (e != hipSuccess) {   // (no kernel may run without its table: off again)
    (void)set_extra_tally(h, EXTRA_PATH_BINS, false);
    h->binEdges.clear();
    return h->hipfail("i3rc_hip_set_path_histogram: uploading the bin edges", e);
  }
  return 0;
}

int i3rc_hip_get_path_histogram_layout(const i3rc_hip_integrator *h, int64_t *binUp, int64_t *binPathUp, int64_t *binDown, int64_t *binPathDown,
                                       int64_t *nBins, int64_t *total) {
  if (!h) return 1;
  const bool on = h->extra == EXTRA_PATH_BINS;
  const int64_t block = extra_block_offset(h->layout.counters);
  int64_t *const out[4] = {binUp, binPathUp, binDown, binPathDown};
  for (int f = 0; f < 4; ++f)
    if (out[f]) *out[f] = on ? block + path_bin_field(f, h->pathBins) : -1;
  if (nBins) *nBins = on ? h->pathBins : 0;
  if (total) *total = h->layout.total;
  return 0;
}

/* Tunables for experiments (not part of the reference API): event-phase ballot threshold, blocks per CU. */
int i3rc_hip_set_tuning(i3rc_hip_integrator *h, int evThreshold, int blocksPerCU) {
  if (!h) return 1;
  drop_lookahead(h);
  if (evThreshold >= 0 && evThreshold <= 64) h->evThreshold = evThreshold;   // 0 = default
  if (blocksPerCU >= 0 && blocksPerCU <= 8) h->blocksPerCU = blocksPerCU;
  return 0;
}

/* Test / measurement knob: plain launches of the specialised flux kernels land a zenith sun's photons from the column table (1, the
 * default) or fly every photon step by step (0); the results are the same word for word.  I3RC_FIRST_FLIGHT_TABLE=0 in the
 * environment is "off" for the process. */
int i3rc_hip_set_first_flight_table(i3rc_hip_integrator *h, int on) {
  if (!h) return 1;
  drop_lookahead(h);
  h->flightOn = on != 0;
  return 0;
}

/* Test hook: 1 where the most recent launch landed its photons from the column table (the bit kFirstFlight of its eventFlags), else 0. */
int i3rc_hip_last_first_flight(const i3rc_hip_integrator *h) { return h && h->lastLanded ? 1 : 0; }

int i3rc_hip_set_light_threshold(i3rc_hip_integrator *h, int lanes) {
  if (!h) return 1;
  drop_lookahead(h);
  if (lanes < 0 || lanes > 64) return h->fail("i3rc_hip_set_light_threshold: need 1..64 lanes (0 = default)");
  h->lightThreshold = lanes;
  return 0;
}

int i3rc_hip_set_launch_limit(i3rc_hip_integrator *h, int64_t photons) {
  if (!h) return 1;
  drop_lookahead(h);
  if (photons < 0) return h->fail("i3rc_hip_set_launch_limit: negative limit");
  h->launchLimit = photons;
  return 0;
}

int i3rc_hip_select_kernel(i3rc_hip_integrator *h, int variant) {
  if (!h) return 1;
  drop_lookahead(h);
  if (variant < I3RC_KERNEL_AUTO || variant > I3RC_KERNEL_RING) return h->fail("i3rc_hip_select_kernel: unknown variant");
  h->kernelVariant = variant;
  return 0;
}

int i3rc_hip_select_grid_place(i3rc_hip_integrator *h, int place) {
  if (!h) return 1;
  drop_lookahead(h);
  if (place < I3RC_GRID_AUTO || place > I3RC_GRID_COLUMNS) return h->fail("i3rc_hip_select_grid_place: unknown place");
  if (place == I3RC_GRID_COLUMNS && !h->colRecords)
    return h->fail("i3rc_hip_select_grid_place: the field has no column records (some column holds more than one run of one value)");
  if (place == I3RC_GRID_BRICKS && h->nz > 65534) return h->fail("i3rc_hip_select_grid_place: more than 65534 layers keep the linear field");
  h->gridPlace = place;
  return 0;
}

int i3rc_hip_has_column_records(const i3rc_hip_integrator *h) { return h && h->colRecords ? 1 : 0; }

/* Column records (DevProblem::colRec) of a field [nz][ny][nx]: possible when the cells with extinction of every column are ONE run
 * of layers that hold ONE value -- compared bit by bit; "no extinction" is the bit pattern of +0, which is what a record gives
 * outside its run (a -0, a NaN or a negative value is "something there" and must be the run's value like any other).  Host code
 * only.  records (may be NULL): [ny * nx][2] words -- the value's bits; first layer (1-based) | (run length - 1) << 16; a clear
 * column is the value 0 in layer 1.  Returns 1 when the field has the form, 0 when it has not (or has more than 65534 layers). */
int i3rc_hip_column_records(int nx, int ny, int nz, const float *totalExt, uint32_t *records) {
  if (nx < 1 || ny < 1 || nz < 1 || !totalExt || nz > 65534) return 0;
  const size_t ncol = (size_t)nx * ny;
  for (size_t c = 0; c < ncol; ++c) {
    uint32_t val = 0u; int first = 0, last = 0;   // 1-based layers of the run
    for (int k = 0; k < nz; ++k) {
      uint32_t bits; std::memcpy(&bits, &totalExt[(size_t)k * ncol + c], sizeof(bits));
      if (bits == 0u) continue;
      if (first == 0) { val = bits; first = last = k + 1; }
      else if (bits == val && last == k) last = k + 1;
      else return 0;
    }
    if (records) {
      records[2 * c] = val;
      records[2 * c + 1] = first == 0 ? 1u : ((uint32_t)first | ((uint32_t)(last - first) << 16));
    }
  }
  return 1;
}

/* Column records OVER A BASE PROFILE (DevProblem::colBase): the field is base(z) + (z within the column's run ? value(x, y) : 0) in
 * float32 arithmetic -- what a cloud scene of one run of one value per column and a horizontally uniform second component add up to.
 * base(z) is the smallest value of the layer (some column must be outside its run there); a column's run is where it differs from
 * the base, and its value is looked for among the float32 numbers around (first differing value - base): the one whose float32 sum
 * with the base gives the field's value in EVERY layer of the run, bit by bit.  Host code only.  Returns 1 / 0; records as
 * i3rc_hip_column_records, base[nz]. */
int i3rc_hip_column_records_base(int nx, int ny, int nz, const float *totalExt, uint32_t *records, float *base) {
  if (nx < 1 || ny < 1 || nz < 1 || !totalExt || !base || nz > 65534) return 0;
  const size_t ncol = (size_t)nx * ny;
  auto bits_of = [](float v) { uint32_t b; std::memcpy(&b, &v, sizeof(b)); return b; };
  for (int k = 0; k < nz; ++k) {
    float b = totalExt[(size_t)k * ncol];
    for (size_t c = 1; c < ncol; ++c) b = std::min(b, totalExt[(size_t)k * ncol + c]);
    if (!(b >= 0.0f) || !std::isfinite(b)) return 0;
    base[k] = b;
  }
  for (size_t c = 0; c < ncol; ++c) {
    int first = 0, last = 0;
    for (int k = 0; k < nz; ++k) {
      if (bits_of(totalExt[(size_t)k * ncol + c]) == bits_of(base[k])) continue;
      if (first == 0) first = last = k + 1;
      else if (last == k) last = k + 1;
      else return 0;                       // a second run
    }
    uint32_t val = 0u;
    if (first != 0) {
      const float guess = totalExt[(size_t)(first - 1) * ncol + c] - base[first - 1];
      bool found = false;
      for (int step = 0; step <= 8 && !found; ++step) {   // the candidates: guess + j float32 steps, j = 0, +1, -1, +2, -2, ...
        const int j = (step + 1) / 2 * (step % 2 ? 1 : -1);
        float v = guess;
        for (int t = 0; t < std::abs(j); ++t) v = std::nextafter(v, j > 0 ? INFINITY : -INFINITY);
        if (!(v > 0.0f)) continue;
        bool ok = true;
        for (int k = first - 1; k < last && ok; ++k) {
          volatile float sum = base[k] + v;   // (one float32 addition, as the host that summed the components made it)
          ok = bits_of(sum) == bits_of(totalExt[(size_t)k * ncol + c]);
        }
        if (ok) { val = bits_of(v); found = true; }
      }
      if (!found) return 0;
    }
    if (records) {
      records[2 * c] = val;
      records[2 * c + 1] = first == 0 ? 1u : ((uint32_t)first | ((uint32_t)(last - first) << 16));
    }
  }
  return 1;
}

int i3rc_hip_set_lds_tallies(i3rc_hip_integrator *h, int on) {
  if (!h) return 1;
  drop_lookahead(h);
  h->ldsTalliesOn = on != 0;
  return 0;
}

int i3rc_hip_lds_plan(const int32_t *q, int32_t *out) { return i3rc_hip_lds_plan_words(q, 17, out, 12); }

int i3rc_hip_lds_plan_words(const int32_t *q, int nq, int32_t *out, int nout) {
  if (!q || !out || nq < 17 || nout < 12) return 1;
  DevProblem P;
  std::memset(&P, 0, sizeof(P));
  P.nx = q[0]; P.ny = q[1]; P.nz = q[2]; P.ncomp = q[3]; P.nDir = q[4]; P.ldsTallies = q[5]; P.ldsIntensity = q[6];
  P.rayQueueCap = q[7]; P.clearNx = q[8]; P.clearShift = q[9]; P.ldsVolume = q[16];
  const LdsPlan lp = lds_plan(P, q[10] != 0, q[11] != 0, q[12], q[13] != 0, q[14], q[15], nq > 17 && q[17] != 0);
  const int v[13] = {lp.xE, lp.yE, lp.zE, lp.tallies, lp.dirCos, lp.dirTab, lp.queue, lp.tInt, lp.ext, lp.cosTab, lp.end, lp.tVol, lp.startStore};
  for (int k = 0; k < std::min(nout, 13); ++k) out[k] = v[k];
  return 0;
}

int i3rc_hip_set_batch_fusion(i3rc_hip_integrator *h, int mode) {
  if (!h) return 1;
  drop_lookahead(h);
  if (mode < -1 || mode > 1) return h->fail("i3rc_hip_set_batch_fusion: mode is -1 (automatic), 0 (never) or 1 (whenever possible)");
  h->fusion = mode;
  h->fusedAheadFailed = false;
  return 0;
}

/* Older name of i3rc_hip_select_kernel(h, on ? I3RC_KERNEL_GENERAL : I3RC_KERNEL_AUTO). */
int i3rc_hip_force_general_kernel(i3rc_hip_integrator *h, int on) {
  return i3rc_hip_select_kernel(h, on ? I3RC_KERNEL_GENERAL : I3RC_KERNEL_AUTO);
}

}  // extern "C"

namespace {

// A launch as it goes to the device: what was decided (launch_plan.hpp) and the kernels' view of the problem
struct Launch { LaunchDecision d; DevProblem P; };

// The geometry of the domain and its extinction field in every packed form: what tracing alone needs of a DevProblem.
void fill_geometry(const i3rc_hip_integrator *h, DevProblem &P) {
  std::memset(&P, 0, sizeof(P));
  P.nx = h->nx; P.ny = h->ny; P.nz = h->nz; P.ncomp = h->ncomp;
  P.xyRegular = h->xyRegular; P.zRegular = h->zRegular;
  P.x0 = h->xE.front(); P.xMax = h->xE.back();
  P.y0 = h->yE.front(); P.yMax = h->yE.back();
  P.z0 = h->zE.front(); P.zMax = h->zE.back();
  P.deltaX = h->xE[1] - h->xE[0]; P.deltaY = h->yE[1] - h->yE[0]; P.deltaZ = h->zE[1] - h->zE[0];
  P.xE = (const float *)h->dxE.p; P.yE = (const float *)h->dyE.p; P.zE = (const float *)h->dzE.p;
  P.colRec = (const uint2 *)h->dColRec.p; P.colBase = (const float *)h->dColBase.p;
  P.extBrick = (const float *)h->dExtBrick.p;
  P.bsx = h->bsx; P.bsy = h->bsy; P.bsz = h->bsz; P.nbx = h->nbx; P.nbxy = h->nbx * h->nby;
  P.clearMap = (const uint32_t *)h->dClearMap.p; P.clearShift = h->clearShift; P.clearNx = h->clearNx;
  P.totalExt = (const float *)h->dExt.p;
}

// The DevProblem of a launch that `d` has decided (not refused).  (stream: where the launch goes, tally: the buffer it adds to)
int first_flight(i3rc_hip_integrator *h, const LaunchDecision &d, DevProblem &P, const RunArgs &A, hipStream_t stream);
// (A: the launch's source, already uploaded -- what the first flight's eligibility reads of it)
int make_problem(i3rc_hip_integrator *h, const LaunchDecision &d, DevProblem &P, const RunArgs &A, hipStream_t stream, double *tally) {
  fill_geometry(h, P);
  // (the kernels take the packed form of the decision's place, and no other)
  if (d.place != GRID_COLUMNS && d.place != GRID_COLBASE) P.colRec = nullptr;
  if (d.place != GRID_COLBASE) P.colBase = nullptr;
  if (d.place != GRID_BRICKS) P.extBrick = nullptr;
  P.cumExt = (const float *)h->dCum.p; P.ssa = (const float *)h->dSsa.p;
  P.pfIndex = (const int32_t *)h->dPf.p;
  P.cellRec = (const uint4 *)h->dCellRec.p;
  if (h->compDirty) {
    // the device copy of the table descriptors follows the host copy when a table was (re)set: a blocking copy after
    // the stream has drained (launches in flight read the old descriptors), not an asynchronous copy from the
    // pageable handle per launch
    if (hipStreamSynchronize(stream) != hipSuccess ||
        hipMemcpy(h->dComp.p, h->comp.data(), sizeof(CompTables) * h->ncomp, hipMemcpyHostToDevice) != hipSuccess)
      return h->fail("copying the component table descriptors failed");
    h->compDirty = false;
  }
  P.comp = (const CompTables *)h->dComp.p;
  P.comp0 = h->comp[0];
  P.albedo = h->params.surfaceAlbedo; P.useBDRF = h->params.useSurfaceBDRF;
  if (uniform_surface(*h)) { P.albedo = h->brdf0; P.useBDRF = 0; }
  P.nxs = h->nxs; P.nys = h->nys;
  P.xsE = (const float *)h->dXs.p; P.ysE = (const float *)h->dYs.p; P.brdf = (const float *)h->dBrdf.p;
  P.useRayTracing = traced(*h) ? 1 : 0; P.useRR = h->params.useRussianRoulette;
  P.nDir = h->nDir; P.useHybrid = h->params.useHybridPhaseFunsForIntenCalcs;
  P.numOrdersOrig = h->params.numOrdersOrigPhaseFunIntenCalcs; P.useRRI = h->params.useRussianRouletteForIntensity;
  P.limitContrib = h->params.limitIntensityContributions; P.zetaMin = h->params.zetaMin;
  P.maxContrib = h->params.maxIntensityContribution; P.maxExt = h->maxExt;
  P.dirCos = (const float *)h->dDir.p;
  // (the path histogram's launches have no radiance directions -- extra_tally_refused --: the pointer carries the bin table, BinTable)
  if (h->extra == EXTRA_PATH_BINS && h->nDir == 0) P.dirCos = (const float *)h->dBins.p;
  P.uniformSsa = h->uniformSsa; P.uniformPf = h->uniformPf;
  P.eventFlags = event_flags(P.uniformSsa, P.uniformPf, P.useBDRF != 0, P.albedo, P.useRR != 0);
  P.tally = tally;
  const TallyView &V = h->view;
  P.oUp = (int)V.fluxUp; P.oDown = (int)V.fluxDown; P.oAbs = (int)V.fluxAbsorbed; P.oVol = (int)V.volumeAbsorption;
  P.oInt = (int)V.intensityByComponent; P.oExc = (int)V.intensityExcess; P.oCnt = (int)V.counters;
  P.rayQueueCap = d.rayQueueCap;
  P.ldsTallies = d.ldsTallies; P.ldsVolume = d.ldsVolume; P.ldsIntensity = d.ldsIntensity; P.ldsGrid = d.ldsGrid | (d.ldsBins ? kLdsGridBinSums : 0);
  // (last: the bit kFirstFlight of eventFlags and, with it, the column table in dirCos -- first_flight, below)
  return first_flight(h, d, P, A, stream);
}

// fluxAbsorbed(ix, iy) of a tally block = the sum of its column's volumeAbsorption (:644-647 add the same increment to both; the kernels
// tally the cell only: Tally::absorbed).  An assignment: a block that several launches add to is summed again after each of them.
__global__ void __launch_bounds__(256) absorbed_columns_kernel(double *blocks, long long stride, int oAbs, int oVol, int ncol, int nz) {
  const int col = (int)(blockIdx.x * 256 + threadIdx.x);
  if (col >= ncol) return;
  double *const blk = blocks + (size_t)blockIdx.y * stride;
  double s = 0.0;
  for (int k = 0; k < nz; ++k) s += blk[oVol + (size_t)k * ncol + col];
  blk[oAbs + col] = s;
}
int absorbed_columns(i3rc_hip_integrator *h, hipStream_t stream, double *blocks, int nBlocks, long long stride) {
  if (!h->absorbing || nBlocks < 1) return 0;   // (nothing absorbs: both tallies stay zero)
  const int ncol = h->nx * h->ny;
  for (int first = 0; first < nBlocks; first += 65535) {
    const int n = std::min(65535, nBlocks - first);
    hipLaunchKernelGGL(absorbed_columns_kernel, dim3((unsigned)((ncol + 255) / 256), (unsigned)n), dim3(256), 0, stream, blocks + (size_t)first * stride,
                       stride, (int)h->view.fluxAbsorbed, (int)h->view.volumeAbsorption, ncol, h->nz);
    HIPCHK(h, hipGetLastError());
  }
  return 0;
}

int upload_source(i3rc_hip_integrator *h, const i3rc_source *src, int64_t n, RunArgs &A) {
  A.srcKind = src->kind;
  if (src->kind == 0) {
    if (std::fabs(src->solarMu) > 1.f || std::fabs(src->solarMu) <= FLT_MIN) return h->fail("setIllumination: solarMu out of bounds");
    if (src->solarAzimuth < 0.f || src->solarAzimuth > 360.f) return h->fail("setIllumination: solarAzimuth out of bounds");
    A.solarMu = -std::fabs(src->solarMu);                      // Code/monteCarloIllumination.f95:98
    A.solarPhi = src->solarAzimuth * std::acos(-1.0f) / 180.f; // :99
    // makeDirectionCosines (:2041-2059) once on the host: the same libm float32 calls the reference makes
    const float sinTheta = std::sqrt(1.0f - A.solarMu * A.solarMu);
    A.solarDx = sinTheta * std::cos(A.solarPhi);
    A.solarDy = sinTheta * std::sin(A.solarPhi);
    A.solarDz = A.solarMu;
    return 0;
  }
  if (src->kind != 1) return h->fail("unknown photon source kind");
  const float *arrs[5] = {src->x, src->y, src->z, src->mu, src->phi};
  const float **dst[5] = {&A.sx, &A.sy, &A.sz, &A.smu, &A.sphi};
  for (int k = 0; k < 5; ++k) if (!arrs[k]) return h->fail("explicit photon stream: null array");
  // what the reference's photon-stream constructors check (Code/monteCarloIllumination.f95:78-83, :124, :204, :369-371):
  // relative positions within [0, 1], |mu| in (tiny, 1] -- a horizontal or NaN direction would never leave the domain
  for (int64_t i = 0; i < n; ++i) {
    const float mu = src->mu[i];
    if (!(std::fabs(mu) <= 1.f) || !(std::fabs(mu) > FLT_MIN)) return h->fail("setIllumination: solarMu out of bounds");
    if (!(src->x[i] >= 0.f && src->x[i] <= 1.f) || !(src->y[i] >= 0.f && src->y[i] <= 1.f) || !(src->z[i] >= 0.f && src->z[i] <= 1.f))
      return h->fail("setIllumination: photon position out of bounds (relative positions lie in [0, 1])");
    if (!std::isfinite(src->phi[i])) return h->fail("setIllumination: solarAzimuth out of bounds");
  }
  for (int k = 0; k < 5; ++k) {
    HIPCHK(h, h->srcBuf[k].upload(arrs[k], sizeof(float) * (size_t)n));
    *dst[k] = (const float *)h->srcBuf[k].p;
  }
  return 0;
}

// THE FIRST FLIGHT (first_flight.hpp): a launch that first_flight_eligible accepts gets the bit kFirstFlight in its eventFlags and the
// column table in DevProblem::dirCos (a launch of a STORE kernel has no radiance directions: nobody else reads the pointer).
// The table depends on the domain alone -- the field, the edges, the Directional start height -- and is made ONCE per integrator: at
// the first launch that could use it, on that launch's stream, not at create.  Create does not know the source: most integrators of
// an oblique sun, of radiances or of explicit photon streams would pay ncol * (nz + 1) words and a kernel for nothing.  The one wait
// for the stream (the sweep's verdict decides the launch's bit on the host) falls into a driver's first batch; a driver keeps its
// integrator for all its batches.  A table beyond kFlightTableMax bytes is not made.
constexpr size_t kFlightTableMax = (size_t)256 << 20;
// Makes the table on `stream` and waits for the sweep's verdict.  0: the table is there and `layer` is the start layer its kernel found,
// `fit` whether a launch may land from it; else a HIP error, the table freed.
hipError_t make_flight_table(i3rc_hip_integrator *h, const DevProblem &P, hipStream_t stream, int &layer, bool &fit) {
#if I3RC_FIRST_FLIGHT_TABLE != 0
  const size_t ncol = (size_t)P.nx * P.ny;
  DevBuf info;
  int words[2] = {0, 1};
  hipError_t e = h->dFlight.alloc(sizeof(float) * ncol * (size_t)(P.nz + 1));
  if (e == hipSuccess) e = info.alloc(sizeof(words));
  if (e == hipSuccess) e = hipMemsetAsync(info.p, 0, sizeof(words), stream);
  if (e == hipSuccess) {
    const size_t lds = sizeof(float) * (size_t)(P.nx + P.ny + P.nz + 3);
    hipLaunchKernelGGL(first_flight_table_kernel, dim3((unsigned)((ncol + 255) / 256)), dim3(256), lds, stream, P, (float *)h->dFlight.p, (int *)info.p);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(words, info.p, sizeof(words), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { h->dFlight.release(); return e; }
  layer = words[0]; fit = words[1] == 0;
  return hipSuccess;
#else
  (void)h; (void)P; (void)stream; (void)layer; (void)fit;
  return hipSuccess;
#endif
}
// flightState: 0 no verdict yet -- the next launch that could use the table makes it, also after an attempt that ended in a HIP error
// (out of memory, say: the launch then flies its photons as before, and nothing stays allocated) --, 1 made and fit, 2 for good no
// table: too large, or its sweep met what makes it unfit (freed).
int first_flight(i3rc_hip_integrator *h, const LaunchDecision &d, DevProblem &P, const RunArgs &A, hipStream_t stream) {
  h->lastLanded = false;
#if I3RC_FIRST_FLIGHT_TABLE != 0
  const bool store = d.startStore && P.nDir == 0;
  if (!h->flightOn || !EnvKnobs::process().firstFlight) return 0;
  // (everything but the table's own verdict first: no table for a launch that could not use it)
  if (!first_flight_eligible(store, A.srcKind, A.solarDx, A.solarDy, A.solarDz, 1, P.nx, P.ny, P.nz, true)) return 0;
  if (h->flightState == 0 && P.totalExt != nullptr) {
    const size_t bytes = sizeof(float) * (size_t)P.nx * P.ny * (size_t)(P.nz + 1);
    if (bytes > kFlightTableMax) h->flightState = 2;
    else {
      bool fit = false;
      if (make_flight_table(h, P, stream, h->flightLayer, fit) == hipSuccess) {
        h->flightState = fit ? 1 : 2;
        if (!fit) h->dFlight.release();
      } else (void)hipGetLastError();   // (the error is the table's alone: this launch flies its photons as before, the next one tries again)
    }
  }
  if (first_flight_eligible(store, A.srcKind, A.solarDx, A.solarDy, A.solarDz, h->flightLayer, P.nx, P.ny, P.nz, h->flightState == 1)) {
    P.eventFlags |= kFirstFlight;
    h->lastLanded = true;
    P.dirCos = (const float *)h->dFlight.p;
  }
#else
  (void)h; (void)d; (void)P; (void)A; (void)stream;
#endif
  return 0;
}

// A launch's decision, its DevProblem and its source, in the order a call reports what it refuses: the problem's completeness, the
// source (upload_source), then LDS.
int prepare_launch(i3rc_hip_integrator *h, const StreamKind &s, const i3rc_source *src, int64_t n, hipStream_t stream, double *tally,
                   Launch &L, RunArgs &A) {
  L.d = plan_launch(*h, EnvKnobs::process(), {s, src->kind});
  if (!L.d.refusal.empty() && L.d.early) return h->fail(L.d.refusal);
  if (upload_source(h, src, n, A)) return 1;
  if (!L.d.refusal.empty()) return h->fail(L.d.refusal);
  return make_problem(h, L.d, L.P, A, stream, tally);
}

// A production instantiation of photon_kernel: its template arguments after the stream -- the key a launch looks it up by --, the kernel
// and its name, formatted from the same arguments in the form tools/kernel_resources.demangle_photon_kernel gives the code object's
// symbol.  lastKernelName is set from the entry that is launched, so a name a test asserts on is the kernel that ran.
using Kernel = void (*)(DevProblem, RunArgs, int, int);
struct KernelEntry {
  KernelKey key;
  Kernel fn;
  const char *name;
};

template <class Rng>
constexpr const char *rng_name() {
  if constexpr (Rng::kExtra == EXTRA_LEVELS) return "PhiloxLevelStream";
  else if constexpr (Rng::kExtra == EXTRA_TRACKS) return "PhiloxTrackStream";
  else if constexpr (Rng::kExtra == EXTRA_PATHS) return "PhiloxPathStream";
  else if constexpr (Rng::kExtra == EXTRA_PATH_BINS) return "PhiloxBinStream";
  else if constexpr (Rng::kExtra == EXTRA_RADIANCE_PATHS) return "PhiloxRadiancePathStream";
  else if constexpr (Rng::kReplay) return "ReplayStream";
  else if constexpr (Rng::kBatched) return "PhiloxBatchStream";
  else return "PhiloxStream";
}

template <class Rng, bool INTENSITY, bool GENERAL, int GRID, bool TBL, bool DIRECT, bool MULTI>
KernelEntry entry() {
  static const char *const placeName[5] = {"GRID_LDS", "GRID_GLOBAL", "GRID_BRICKS", "GRID_COLUMNS", "GRID_COLBASE"};
  static const std::string name = std::string("photon_kernel<") + rng_name<Rng>() + (INTENSITY ? ", true" : ", false") +
                                  (GENERAL ? ", true, " : ", false, ") + placeName[GRID] + (TBL ? ", table in LDS" : "") +
                                  (DIRECT ? ", one direction" : "") + (MULTI ? ", wide" : "") + ">";
  return {{INTENSITY, GENERAL, GRID, TBL, DIRECT, MULTI}, photon_kernel<Rng, INTENSITY, GENERAL, GRID, TBL, DIRECT, MULTI>, name.c_str()};
}

// the instantiation at each of the places GRID... of the extinction field
template <class Rng, bool INTENSITY, bool GENERAL, bool TBL, bool DIRECT, bool MULTI, int... GRID>
void add(std::vector<KernelEntry> &v, std::integer_sequence<int, GRID...>) {
  (..., v.push_back(entry<Rng, INTENSITY, GENERAL, GRID, TBL, DIRECT, MULTI>()));
}
using AllPlaces = std::integer_sequence<int, GRID_LDS, GRID_GLOBAL, GRID_BRICKS, GRID_COLUMNS, GRID_COLBASE>;
// (GRID_COLBASE -- column records over a base profile -- exists for the kernels that run domains of several components: the general
// ones and the widened ones; plan_launch never plans it for anything else, nor for the replay build)
using NoColbase = std::integer_sequence<int, GRID_LDS, GRID_GLOBAL, GRID_BRICKS, GRID_COLUMNS>;

// The production instantiations, once per stream.  Template arguments after the stream: INTENSITY, GENERAL, TBL, DIRECT, MULTI.
template <class Rng>
const std::vector<KernelEntry> &stream_kernels() {
  static const std::vector<KernelEntry> list = [] {
    std::vector<KernelEntry> v;
    if constexpr (Rng::kExtra == EXTRA_RADIANCE_PATHS) {   // the radiance path tally: the general radiance kernel, at every place
      add<Rng, true, true, false, false, false>(v, AllPlaces{});
    } else if constexpr (Rng::kExtra != EXTRA_NONE) {   // an extra tally block: the general flux kernel, at every place
      add<Rng, false, true, false, false, false>(v, AllPlaces{});
    } else if constexpr (Rng::kBatched) {   // fused multi-batch launches
      add<Rng, false, false, false, false, false>(v, NoColbase{});   // flux, the common class
      add<Rng, false, false, false, false, true>(v, AllPlaces{});    // the widened class: flux, ...
      add<Rng, true, false, false, false, true>(v, AllPlaces{});     // ... radiance through the event ring, ...
      add<Rng, true, false, false, true, true>(v, AllPlaces{});      // ... one radiance direction
      add<Rng, true, false, false, false, false>(v, NoColbase{});    // radiance through the event ring
      add<Rng, true, false, false, true, false>(v, NoColbase{});     // one radiance direction
      add<Rng, false, false, true, false, false>(v, std::integer_sequence<int, GRID_LDS, GRID_GLOBAL, GRID_COLUMNS>{});   // flux, table in LDS
    } else if constexpr (!Rng::kReplay) {
      add<Rng, false, true, false, false, false>(v, AllPlaces{});    // the general kernels: flux, ...
      add<Rng, true, true, false, false, false>(v, AllPlaces{});     // ... radiance through the event ring
      add<Rng, false, false, false, false, false>(v, NoColbase{});   // the common class: flux, ...
      add<Rng, true, false, false, false, false>(v, NoColbase{});    // ... radiance through the event ring
      add<Rng, true, false, false, false, true>(v, AllPlaces{});     // the widened class: radiance through the event ring, ...
      add<Rng, true, false, false, true, true>(v, AllPlaces{});      // ... one radiance direction
      add<Rng, true, true, false, true, false>(v, AllPlaces{});      // one radiance direction: general, ...
      add<Rng, true, false, false, true, false>(v, NoColbase{});     // ... the common class
      add<Rng, false, false, true, false, false>(v, NoColbase{});    // flux, the common class, table in LDS
    } else {   // (the replay build runs the general kernels only)
      add<Rng, false, true, false, false, false>(v, NoColbase{});
      add<Rng, true, true, false, false, false>(v, NoColbase{});
    }
    return v;
  }();
  return list;
}

// An extra tally block is filled by the general flux kernel of a plain launch, traced: what a launch must be while one is switched on.
// Called before a launch touches anything; `who` names the entry point in the error text, `batches` says that it runs a loop of
// batches (fused or announced), which no such kernel serves.
// (path lengths have no batch statistics: the diagnostic moments' layout has no slot for them)
std::string no_path_moments_text() {
  return "path lengths have no batch statistics; the diagnostic moments' layout has no slot for them (switch them off, or call "
         "i3rc_hip_launch_batch / i3rc_hip_compute_batch per batch; i3rc_hip_run_batches_path_moments gathers them in a layout of its own)";
}
// (nor has the path histogram)
std::string no_bin_moments_text() {
  return "the path histogram has no batch statistics; the diagnostic moments' layout has no slot for it (switch it off, or call "
         "i3rc_hip_launch_batch / i3rc_hip_compute_batch per batch; i3rc_hip_run_batches_path_moments gathers them in a layout of its own)";
}
// (nor have the radiance path lengths, yet)
std::string no_radiance_path_moments_text() {
  return "radiance path lengths have no batch statistics yet; no moments layout has a slot for them (switch them off, or call "
         "i3rc_hip_launch_batch / i3rc_hip_compute_batch per batch)";
}
int extra_tally_refused(i3rc_hip_integrator *h, const char *who, bool batches) {
  if (h->extra == EXTRA_NONE) return 0;
  const ExtraWords &w = kExtraWords[h->extra];
  const std::string subject = std::string(who) + ": " + w.noun + " ";
  if (h->extra == EXTRA_RADIANCE_PATHS) {   // the one kind of the general RADIANCE kernel
    if (batches)
      return h->fail(subject + "have no batch statistics yet and are tallied by plain launches only; fused or announced batches cannot give them "
                               "(switch them off, or call i3rc_hip_launch_batch / i3rc_hip_compute_batch per batch)");
    if (h->nDir < 1) return h->fail(subject + "are tallied by radiance launches only; no radiance direction is set (nDir = 0)");
    for (int d = 0; d < h->nDir; ++d)
      if (!(h->dirHost[3 * (size_t)d + 2] > 0.0f))
        return h->fail(subject + "need upward radiance directions; direction " + std::to_string(d + 1) + " has uz <= 0 (its rays never reach the top)");
    if (!traced(*h)) return h->fail(subject + "need ray tracing; max cross-section is in use (useRayTracing = 0)");
    if (h->params.limitIntensityContributions)
      return h->fail(subject + "cannot follow limited contributions; the redistributed excess has no path (limitIntensityContributions = 1)");
    return 0;
  }
  if (batches)
    return h->fail(subject + w.are + " tallied by plain launches only; fused or announced batches cannot give " + w.them + " (switch " + w.them +
                   " off, or call i3rc_hip_launch_batch / i3rc_hip_compute_batch per batch)");
  if (h->nDir > 0) return h->fail(subject + w.are + " tallied by flux launches only; radiance directions are set (nDir > 0)");
  if (!h->params.useRayTracing) return h->fail(subject + w.need + " ray tracing; max cross-section is in use (useRayTracing = 0)");
  return 0;
}

const char *no_kernel_text(bool fused) {
  return fused ? "internal: no fused kernel for this problem at this place of the extinction field"
               : "internal: no kernel for this problem at this place of the extinction field";
}

// One grid of the kernel decided for the launch on `stream`: the record of the launch (lastKernelName, i3rc_hip_last_plan),
// occupancy and block count, then `prepare(blocks, threads)` -- what the caller puts on the stream in front of the kernel, and may
// change A -- and the launch between the events of the timing ring.  fusedBatches: the batches of a fused launch (0: a plain one).
template <class Rng, class Prepare>
int launch_grid(i3rc_hip_integrator *h, const Launch &L, RunArgs &A, hipStream_t stream, int fusedBatches, bool timeIt, Prepare &&prepare) {
  const KernelEntry *kern = nullptr;
  for (const KernelEntry &e : stream_kernels<Rng>())
    if (e.key == L.d.key) kern = &e;
  if (!kern) return h->fail(no_kernel_text(Rng::kBatched));
  const int threads = L.d.threads;
  const size_t ldsBytes = L.d.ldsBytes;
  const void *fn = (const void *)kern->fn;
  h->lastKernelName = kern->name;
  plan_words(*h, L.d, fusedBatches, h->lastPlan);
  h->lastPlanBins = L.d.ldsBins;
  int perCU = h->blocksPerCU;
  if (perCU <= 0) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, ldsBytes) != hipSuccess || occ < 1) occ = 2;
    perCU = std::min(occ, 8);
    // a field beyond an XCD's L2 (bricks): every wave in flight widens the part of it that is in use; measured on the
    // 7.8 MB Landsat-119 field (tools/blocks_sweep.py): 4-5 workgroups per CU 6.17e8 photons/s, 6-8 5.83e8.  (The radiance
    // kernels have the registers for five at most; fields within L2 gain up to 7.)
    // With the XCD-aware photon order: Landsat-119 5 ... 8 alike (6.5e8); the scene tiled 2 x 2 (31 MB): 4 workgroups 5.41e8,
    // 5 5.02e8, 6-8 4.6e8.
    if (L.d.place == GRID_BRICKS) perCU = std::min(perCU, ncell_bytes(*h) > ((size_t)16 << 20) ? 4 : 5);
  }
  if (ldsBytes > 48 * 1024)
    HIPCHK(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsBytes));
  long long blocks = (long long)h->numCU * perCU;
  const long long photons = fusedBatches > 0 ? (long long)fusedBatches * A.nPhotons : A.nPhotons;
  const long long need = (photons + threads - 1) / threads;
  if (blocks > need) blocks = std::max(1ll, need);
  if (prepare(blocks, threads)) return 1;
  h->lastPlan[kPlanChunk] = A.chunk;   // (photons -- fused launches: per chunk number -- a wave takes per visit of the work counter)
  const int slot = (int)(h->timedLaunches % i3rc_hip_integrator::kEventRing);
  if (timeIt) HIPCHK(h, hipEventRecord(h->evStart[slot], stream));
  {
    // thresholds the caller did not fix are adapted per wave (photon_kernel); negative = adaptive, starting value
    const int evThreshold = h->evThreshold > 0 ? h->evThreshold : -40;
    const int lightThreshold = h->lightThreshold > 0 ? h->lightThreshold : -24;
    hipLaunchKernelGGL(kern->fn, dim3((unsigned)blocks), dim3(threads), ldsBytes, stream, L.P, A, evThreshold, lightThreshold);
  }
  HIPCHK(h, hipGetLastError());
  if (timeIt) { HIPCHK(h, hipEventRecord(h->evStop[slot], stream)); h->timedLaunches++; }
  return 0;
}

template <class Rng>
int launch(i3rc_hip_integrator *h, const Launch &L, const RunArgs &A, hipStream_t stream, bool timeIt) {
  RunArgs B = A;   // photon indices are handed to waves in chunks (one returning atomic per chunk)
  const int rc = launch_grid<Rng>(h, L, B, stream, 0, timeIt, [&](long long blocks, int threads) -> int {
    // XCD-aware photon order.  A field beyond an XCD's L2 (bricks) is shared by eight L2s that each see all of it: when
    // the photons a wave traces start in "its" eighth of the domain -- workgroups are dealt round-robin over the XCDs, the
    // kernel reads its XCC id -- an XCD's L2 has an eighth of the field (and its surroundings) to hold.  The launch's
    // photons are sorted by start slab first (their start position is their own first Philox block): two passes over the
    // photon numbers, about 1 % of the launch.  Radiance runs: local-estimate rays cross much of the domain, but from one
    // tile they keep to a tube per direction -- nothing gained on the 7.8 MB Landsat field (9.49 against 9.45e7 photons/s:
    // left in index order), +20 % on a 31 MB field (6.9 -> 8.3e7 with 7 directions).
    // Measured ceiling (tools/locality_experiment.py): +9 ... 14 % on the 7.8 MB Landsat field, +36 % on a 62 MB field.
    // I3RC_SLABS=0 switches it off.
    static const bool slabsOn = env_on("I3RC_SLABS");
    B.slabIds = nullptr; B.slabMeta = nullptr;
    if constexpr (!Rng::kReplay) {
      if (slabsOn && L.d.place == GRID_BRICKS && (!L.d.key.intensity || ncell_bytes(*h) > ((size_t)16 << 20)) && A.srcKind == 0 && A.nPhotons >= 1024 && A.nPhotons < ((long long)1 << 32)) {
        auto &sb = h->slabBufs[stream];
        if (sb.ids.bytes < (size_t)A.nPhotons * sizeof(uint32_t)) HIPCHK(h, sb.ids.alloc((size_t)A.nPhotons * sizeof(uint32_t)));
        if (!sb.meta.p || sb.meta.bytes != sizeof(SlabMeta)) HIPCHK(h, sb.meta.alloc(sizeof(SlabMeta)));
        const size_t tableBytes = sizeof(unsigned) * 8 * kSlabSortBlocks;
        if (sb.blockCounts.bytes != tableBytes) { HIPCHK(h, sb.blockCounts.alloc(tableBytes)); HIPCHK(h, sb.blockBase.alloc(tableBytes)); }
        const long long span = ((A.nPhotons + kSlabSortBlocks - 1) / kSlabSortBlocks + 255) / 256 * 256;   // photons per workgroup of the sort
        int tx = 1, ty = 8;   // the squarest of the four tilings (ties: more cuts in y, whose rows are further apart in memory)
        for (int cx = 2; cx <= 8; cx *= 2)
          if ((double)h->nx / cx + (double)h->ny / (8 / cx) < (double)h->nx / tx + (double)h->ny / ty) { tx = cx; ty = 8 / cx; }
        hipLaunchKernelGGL(slab_count_kernel, dim3(kSlabSortBlocks), dim3(256), 0, stream, A.seed0, A.seed1, A.firstPhoton, A.nPhotons, span,
                           tx, ty, (unsigned *)sb.blockCounts.p);
        hipLaunchKernelGGL(slab_scan_kernel, dim3(1), dim3(8), 0, stream, (int)kSlabSortBlocks, (const unsigned *)sb.blockCounts.p,
                           (SlabMeta *)sb.meta.p, (unsigned *)sb.blockBase.p);
        hipLaunchKernelGGL(slab_fill_kernel, dim3(kSlabSortBlocks), dim3(256), 0, stream, A.seed0, A.seed1, A.firstPhoton, A.nPhotons, span,
                           tx, ty, (const unsigned *)sb.blockBase.p, (uint32_t *)sb.ids.p);
        HIPCHK(h, hipGetLastError());
        B.slabIds = (const uint32_t *)sb.ids.p; B.slabMeta = (SlabMeta *)sb.meta.p;
      }
    }
    // at most 256 photons per visit of the work counter: four photon generations of a wave.  Measured (I3RC_CHUNK_MAX, a
    // tuning knob): 128 loses a third (a returning atomic every other generation), 256...448 are equal, 1024 loses
    // 0.5 % on the step cloud and 2-5 % on the radar / Landsat cases to the imbalance at the end of a launch.
    static const long long chunkMax = std::max(64ll, env_int("I3RC_CHUNK_MAX", 256));
    B.chunk = (int)std::min<long long>(chunkMax, std::max<long long>(64, A.nPhotons / (blocks * (threads / 64) * 8)));
    // (a launch that lands first flights keeps a wave's landed steps in thirty bits between two hand-overs of its counters, which
    // fall at every fourth refill at the latest and earlier once the sum passes 2^29: chunks of at most 2^16 photons of at most 1022
    // steps keep what four refills add below 2^28 -- I3RC_CHUNK_MAX is a knob without a bound of its own)
    if ((L.P.eventFlags & kFirstFlight) != 0u) B.chunk = std::min(B.chunk, 1 << 16);
    HIPCHK(h, hipMemsetAsync(A.workCounter, 0, sizeof(unsigned long long), stream));
    return 0;
  });
  if (rc) return 1;
  return absorbed_columns(h, stream, L.P.tally, 1, 0);
}

// ---- fused multi-batch launches ---------------------------------------------------------------------------------------
// out[b][e] = sum over the replicas r of blocks[b * R + r][e]
__global__ void __launch_bounds__(256) reduce_replicas_kernel(const double *blocks, double *out, long long nBlocksOut, int R, long long stride) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nBlocksOut * stride) return;
  const long long b = i / stride, e = i - b * stride;
  const double *src = blocks + (size_t)b * R * stride + e;
  double v = 0.0;
  for (int r = 0; r < R; ++r) v += src[(size_t)r * stride];
  out[i] = v;
}

// counters of batch b of the group = sum over the copies of its counter block (RunArgs::counterBlocks), into the batch's tally block
__global__ void __launch_bounds__(256) reduce_counters_kernel(const double *counterBlocks, double *out, long long nBlocksOut, long long stride, int oCnt) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nBlocksOut * I3RC_NUM_COUNTERS) return;
  const long long b = i / I3RC_NUM_COUNTERS;
  const int k = (int)(i - b * I3RC_NUM_COUNTERS);
  const double *src = counterBlocks + (size_t)b * kCounterReplicas * I3RC_NUM_COUNTERS + k;
  double v = 0.0;
  for (int r = 0; r < kCounterReplicas; ++r) v += src[(size_t)r * I3RC_NUM_COUNTERS];
  out[(size_t)b * stride + oCnt + k] = v;
}

// ---- batch moments on the device (i3rc_hip_run_batches_moments, i3rc_hip_run_batches_diagnostic_moments) ----------------
// A driver only ever wants the first two moments over its batches of what reportResults hands out (monteCarloDriver.f95:
// 300-321, reduced at :333-352): per batch the raw block is normalised by the rule of tally_block.hpp, which i3rc_hip_normalise follows too (:353-395,
// float64, rounded to the reference's real(4)) and x, x^2 are added up per element -- the per-batch blocks never leave the device.
// one normalised field value of a batch; e counts through fluxUp | fluxDown | fluxAbsorbed | volumeAbsorption | intensity
__device__ __forceinline__ float moments_field_value(const TallyView &V, const double *raw, const double *excessSums, long long e) {
  const long long ncol = (long long)V.nx * V.ny, ncell = ncol * V.nz;
  if (e < 3 * ncol) {
    const int which = (int)(e / ncol);
    const long long col = e - which * ncol;
    return normalised_column_flux(V, raw, (which == 0 ? V.fluxUp : (which == 1 ? V.fluxDown : V.fluxAbsorbed)) + col, col);
  }
  e -= 3 * ncol;
  if (e < ncell) {
    const int kz = (int)(e / ncol);
    return normalised_volume_absorption(V, raw, kz, e - kz * ncol);
  }
  e -= ncell;
  const int d = (int)(e / ncol);
  return normalised_intensity(V, raw, excessSums, d, e - d * ncol);
}
// What a moments pass adds up, handed to its two kernels by value: element e of batch b (`raw`: the batch's block), the number of
// fields -- they lie in front of the sums in the order e counts them --, the number of domain means, and for mean q its first
// element and its place in the sums.  V's two arrays are device memory here.
struct BatchFields {   // what reportResults hands out (i3rc_moments_layout)
  TallyView V;
  i3rc_moments_layout L;
  const double *excessSums;   // moments_excess_kernel's, (ncomp + 1) * nDir per batch
  __device__ __forceinline__ float value(const double *raw, int b, long long e) const {
    return moments_field_value(V, raw, excessSums + (size_t)b * ((V.ncomp + 1) * V.nDir), e);
  }
  __host__ __device__ __forceinline__ long long fields() const { return L.absorbedProfile; }   // (fluxUp ... intensity: everything in front of the profile)
  // domain means (:739-742), the absorption profile (:780) and the mean radiances
  __host__ __device__ __forceinline__ int means() const { return 3 + V.nz + V.nDir; }
  __device__ __forceinline__ void mean(int q, long long &first, long long &at) const {
    const long long ncol = (long long)V.nx * V.ny;
    // (the three places read before one is chosen: a choice among the members' addresses would keep a copy of *this in scratch)
    const long long flux[3] = {L.meanFluxUp, L.meanFluxDown, L.meanFluxAbsorbed};
    if (q < 3) { first = q * ncol; at = flux[q]; }
    else if (q < 3 + V.nz) { first = 3 * ncol + (long long)(q - 3) * ncol; at = L.absorbedProfile + (q - 3); }
    else { first = 3 * ncol + ncol * V.nz + (long long)(q - 3 - V.nz) * ncol; at = L.meanIntensity + (q - 3 - V.nz); }
  }
};
struct ExtraFields {   // the optional diagnostic tally: the kind's extra block, normalised by normalised_extra_value (extra_moments_layout)
  TallyView V;
  ExtraTally kind;
  __device__ __forceinline__ float value(const double *raw, int, long long e) const { return normalised_extra_value(V, raw, kind, extra_block_offset(V.counters), e); }
  __host__ __device__ __forceinline__ long long fields() const { return extra_block_words(kind, V.nx, V.ny, V.nz); }
  // one mean per level of levelFluxUp | level of levelFluxDown, or per layer: over the columns of the elements q * ncol ...
  __host__ __device__ __forceinline__ int means() const { return (int)extra_moments_means(kind, V.nz); }
  __device__ __forceinline__ void mean(int q, long long &first, long long &at) const { first = (long long)q * V.nx * V.ny; at = fields() + q; }
};
struct PathFields {   // the two path tallies: the kind's block as ExtraFields hands it out, and what is no plain column mean (path_moments_layout)
  TallyView V;
  ExtraTally kind;
  int nBins, nK;
  const float *edges;        // [nBins + 1], the table bin_add reads (device memory)
  const float *absorption;   // [nK] (device memory)
  __device__ __forceinline__ float value(const double *raw, int, long long e) const { return normalised_extra_value(V, raw, kind, extra_block_offset(V.counters), e); }
  __host__ __device__ __forceinline__ long long fields() const { return path_moments_fields(kind, V.nx, V.ny, nBins); }
  __host__ __device__ __forceinline__ int quantities() const { return path_moments_quantities(kind, nK); }
};
// the sum of v over the 256 threads of a workgroup (what thread 0 returns is used)
__device__ __forceinline__ double workgroup_sum(double v) {
  __shared__ double part[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}
// excessSums[b][(j * nDir + d)] = sum over the columns of intensityByComponent(:, :, d, j) of batch b (one workgroup each)
__global__ void __launch_bounds__(256) moments_excess_kernel(TallyView V, const double *blocks, long long stride, double *excessSums) {
  const int per = (V.ncomp + 1) * V.nDir, b = blockIdx.x / per, jd = blockIdx.x - b * per;
  const size_t ncol = (size_t)V.nx * V.ny;
  const double *f = blocks + (size_t)b * stride + V.intensityByComponent + (size_t)jd * ncol;
  double v = 0.0;
  for (size_t k = threadIdx.x; k < ncol; k += 256) v += f[k];
  v = workgroup_sum(v);
  if (threadIdx.x == 0) excessSums[(size_t)b * per + jd] = v;
}
// fields: one thread per element and SLICE of the group's batches (blockIdx.y; a slice's batches one after the other).  A small domain
// with many batches -- 700 elements x 1e5 batches of a thousand photons -- would otherwise be a few hundred threads walking 1e5 batches
// each, longer than the trace itself (round-4 advisor): the launch cuts the batches into as many slices as fill the chip.
template <class Fields>
__global__ void __launch_bounds__(256) moments_fields_kernel(Fields F, const double *blocks, int count, long long stride, double *sum, double *sumSq) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= F.fields()) return;
  const int perSlice = (count + (int)gridDim.y - 1) / (int)gridDim.y;
  const int b0 = (int)blockIdx.y * perSlice, b1 = min(count, b0 + perSlice);
  double s1 = 0.0, s2 = 0.0;
  for (int b = b0; b < b1; ++b) {
    const double x = (double)F.value(blocks + (size_t)b * stride, b, e);
    s1 += x; s2 += x * x;
  }
  unsafeAtomicAdd(sum + e, s1);
  unsafeAtomicAdd(sumSq + e, s2);
}
// domain means: one workgroup per (batch, mean), float32(sum over the columns / number of columns); the workgroup of a batch's first
// mean also adds the batch's counters to counterTotals (where the caller wants them)
template <class Fields>
__global__ void __launch_bounds__(256) moments_means_kernel(Fields F, const double *blocks, long long stride, double *sum, double *sumSq,
                                                            double *counterTotals) {
  const int nq = F.means(), b = blockIdx.x / nq, q = blockIdx.x - b * nq;
  const double *raw = blocks + (size_t)b * stride;
  const long long ncol = (long long)F.V.nx * F.V.ny;
  long long first, at;
  F.mean(q, first, at);
  double v = 0.0;
  for (long long k = threadIdx.x; k < ncol; k += 256) v += (double)F.value(raw, b, first + k);
  v = workgroup_sum(v);
  if (threadIdx.x == 0) {
    const double x = (double)(float)(v / (double)ncol);
    unsafeAtomicAdd(sum + at, x);
    unsafeAtomicAdd(sumSq + at, x * x);
  }
  if (q == 0 && counterTotals && threadIdx.x < I3RC_NUM_COUNTERS) unsafeAtomicAdd(counterTotals + threadIdx.x, raw[F.V.counters + threadIdx.x]);
}

// the path tallies' other quantities: one workgroup per (batch, quantity), threads striding over the columns or the bins.  Path
// lengths: q = 0 .. 3 the plain column mean of field q, q = 4 .. 7 the domain's ratio of field q - 4's raw sum to the raw sum of fluxUp
// (fields 0, 1) or fluxDown (2, 3).  The histogram: q = which * nK + j, which = 0 .. 3 for spectrumUpLower | UpUpper | DownLower |
// DownUpper at absorption[j], from the raw bins in float64 (path_spectrum_term), per photon of the batch.  One rounding to float32 each.
__global__ void __launch_bounds__(256) path_quantities_kernel(PathFields F, const double *blocks, long long stride, double *sum, double *sumSq) {
  const int nq = F.quantities(), b = blockIdx.x / nq, q = blockIdx.x - b * nq;
  const double *raw = blocks + (size_t)b * stride;
  const long long block = extra_block_offset(F.V.counters), at = F.fields() + q;
  double x;
  if (F.kind == EXTRA_PATHS) {
    const long long ncol = (long long)F.V.nx * F.V.ny;
    if (q < 4) {
      double v = 0.0;
      for (long long k = threadIdx.x; k < ncol; k += 256) v += (double)F.value(raw, b, q * ncol + k);
      v = workgroup_sum(v);
      x = (double)(float)(v / (double)ncol);
    } else {
      const double *path = raw + block + (q - 4) * ncol, *flux = raw + (q < 6 ? F.V.fluxUp : F.V.fluxDown);
      double num = 0.0, den = 0.0;
      for (long long k = threadIdx.x; k < ncol; k += 256) { num += path[k]; den += flux[k]; }
      num = workgroup_sum(num);
      __syncthreads();   // (workgroup_sum's partial sums are read: the second sum writes them again)
      den = workgroup_sum(den);
      x = (double)domain_path_ratio(num, den);
    }
  } else {
    const int which = q / F.nK, nb = F.nBins + 1;
    const double k = (double)F.absorption[q - which * F.nK];
    const double *weight = raw + block + path_bin_field(which < 2 ? 0 : 2, F.nBins), *path = weight + nb;
    double v = 0.0;
    for (int bin = threadIdx.x; bin < nb; bin += 256) {
      double lower, upper;
      path_spectrum_term(F.edges, F.nBins, bin, weight[bin], path[bin], k, lower, upper);
      v += (which & 1) ? upper : lower;
    }
    v = workgroup_sum(v);
    x = (double)(float)(v / raw[F.V.counters + I3RC_CNT_PHOTONS]);
  }
  if (threadIdx.x == 0) {
    unsafeAtomicAdd(sum + at, x);
    unsafeAtomicAdd(sumSq + at, x * x);
  }
}

// Do the batches of a driver's loop -- nBatches of nPhotons each -- share one grid, group by group (see FusedSlot)?  The specialised
// kernels -- the common problem class, production streams --, with or (round 4) without radiance directions: a local-estimate ray
// carries its batch in its info word (photon_kernel).  One long batch alone, or batches of a size at which a launch's tail no longer
// matters, go one launch each.
bool fuse_loop(const i3rc_hip_integrator *h, int64_t nPhotons, int nBatches) {
  static const bool envOff = !env_on("I3RC_FUSED");
  if (envOff || h->fusion == 0) return false;
  // (a batch's tally block beyond 256 MiB -- 3e7 cells -- would make a slot's pinned copy and its blocks unreasonably large: such
  // domains keep one launch per batch, whose tail is a small part of a launch that long anyway)
  static const bool radianceOff = !env_on("I3RC_FUSED_RADIANCE");
  if (h->nDir > 0 && (radianceOff || kNestedBuild)) return false;
  // (round 5: the widened class too -- several components, an irregular x / y grid, a gridded surface: photon_kernel<PhiloxBatchStream, ..., MULTI>)
  return (common_class(*h, 0) || multi_class(*h, 0)) && h->kernelVariant != I3RC_KERNEL_GENERAL && nPhotons < ((int64_t)1 << 31) &&
         h->layout.total * (int64_t)sizeof(double) <= ((int64_t)256 << 20) && (h->fusion == 1 || (nBatches >= 2 && nPhotons <= 20000000));
}

// Replicas of a batch's tally block: enough that the hot words of a small domain (fluxUp / fluxDown of nx * ny columns) are
// spread over some 256 cache lines -- measured (tools/microbench/atomic_rate.hip): 64 hot float64 in one block take 4.1e8
// atomics/s from the whole chip, in 8 blocks 1.7e9, in 64 blocks 1.3e10; the step cloud needs 3.4e9.
int fused_replicas(const i3rc_hip_integrator *h) {
  const int64_t ncol = (int64_t)h->nx * h->ny, hotLines = 2 * ((ncol + 15) / 16);
  return (int)std::max<int64_t>(1, std::min<int64_t>(64, 256 / hotLines));
}

// Batches per group: device memory for the blocks (<= 1 GiB) and the pinned copy (<= 256 MiB) bound it; beyond that a
// group wants some 2.5e8 photons: a group boundary costs about 2.4 ms even with the next group queued behind it (step
// cloud, 300 batches of 1e6 photons: 15 groups 0.38, 6 groups 0.34, 3 groups 0.33, 1 group 0.31 ms per batch).
int fused_group_size(const i3rc_hip_integrator *h, int nBatches, int64_t nPhotons, bool moments = false) {
  const int64_t blockBytes = h->layout.total * 8, R = fused_replicas(h);
  int64_t g = ((int64_t)1 << 30) / (blockBytes * R);
  if (!moments) g = std::min<int64_t>(g, ((int64_t)256 << 20) / blockBytes);   // (moments mode: no pinned copy of the blocks)
  static const int64_t target = env_int("I3RC_FUSED_GROUP_PHOTONS", 250000000ll);
  g = std::min<int64_t>(g, (target + nPhotons - 1) / nPhotons);
  if (h->nDir > 0) g = std::min<int64_t>(g, 1 << kRayBatchBits);   // (a local-estimate ray carries its batch in its info word: RayInfo, tracer.hpp)
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, nBatches));
}

// (`reserve`: batches the slot's buffers are made for at least -- a slot that had to grow later would hipFree / hipMalloc while
// other groups are under way, and both wait for the device: a driver's look-ahead, whose groups grow 8, 16 ... 256, stood still
// for a whole group each time)
int ready_fused_slot(i3rc_hip_integrator *h, i3rc_hip_integrator::FusedSlot &g, int count, int R, int reserve, bool toHost) {
  count = std::max(count, reserve);
  const size_t outBytes = (size_t)count * h->layout.total * sizeof(double);
  // All groups share ONE stream (the first slot's): a kernel trace of groups on streams of their own showed consecutive
  // launches overlapping by 2 ms only -- the next kernel gets its first workgroup slots when the one before drains -- while
  // every launch took 5 ms longer than it does alone: with work pending in a second hardware queue the persistent kernel's
  // waves are time-sliced against it.  One queue exposes a launch's 1.4 ms tail per group and nothing else.
  if (!h->fused[0].stream) HIPCHK(h, hipStreamCreateWithFlags(&h->fused[0].stream, hipStreamNonBlocking));
  g.stream = h->fused[0].stream;
  if (!g.done) HIPCHK(h, hipEventCreateWithFlags(&g.done, hipEventDisableTiming));
  if (!g.traced) HIPCHK(h, hipEventCreateWithFlags(&g.traced, hipEventDisableTiming));
  if (!h->fusedCopyStream) HIPCHK(h, hipStreamCreateWithFlags(&h->fusedCopyStream, hipStreamNonBlocking));
  if (!g.counter.p) HIPCHK(h, g.counter.alloc(sizeof(unsigned long long)));
  if (!g.abortFlag) HIPCHK(h, hipHostMalloc((void **)&g.abortFlag, sizeof(int), hipHostMallocCoherent | hipHostMallocMapped));
  if (toHost && g.pinnedBytes < outBytes) {
    if (g.pinned) { HIPCHK(h, hipHostFree(g.pinned)); g.pinned = nullptr; g.pinnedBytes = 0; }
    HIPCHK(h, hipHostMalloc((void **)&g.pinned, outBytes, hipHostMallocDefault));
    g.pinnedBytes = outBytes;
  }
  if (g.blocks.bytes < outBytes * R) HIPCHK(h, g.blocks.alloc(outBytes * R));
  if (R > 1 && g.compact.bytes < outBytes) HIPCHK(h, g.compact.alloc(outBytes));
  const size_t cntBytes = (size_t)count * kCounterReplicas * I3RC_NUM_COUNTERS * sizeof(double);
  if (g.counterBlocks.bytes < cntBytes) HIPCHK(h, g.counterBlocks.alloc(cntBytes));
  return 0;
}

// One group: `count` batches with the keys (seed0, seed1 .. seed1 + count - 1), nPhotons photons each, traced by ONE grid;
// zero, trace, sum the replicas, copy to the slot's pinned buffer -- all asynchronous on the slot's stream.
int accumulate_moments(i3rc_hip_integrator *h, hipStream_t stream, const double *blocks, int count, DevBuf &excess);

// (moments: the group's blocks stay on the device -- normalised and added to the handle's moment sums there, see accumulate_moments)
int launch_fused_group(i3rc_hip_integrator *h, i3rc_hip_integrator::FusedSlot &g, uint32_t seed0, uint32_t seed1, int count,
                       int64_t nPhotons, const i3rc_source *src, bool timeIt, int reserve = 0, bool moments = false) {
  const int R = fused_replicas(h);
  if (ready_fused_slot(h, g, count, R, reserve, !moments)) return 1;
  Launch L;
  RunArgs A;
  std::memset(&A, 0, sizeof(A));
  A.seed0 = seed0; A.seed1 = seed1; A.firstPhoton = 0; A.nPhotons = nPhotons;
  A.workCounter = (unsigned long long *)g.counter.p;
  if (prepare_launch(h, stream_of<PhiloxBatchStream>(), src, nPhotons, g.stream, (double *)g.blocks.p, L, A)) return 1;
  // (chunks: a wave takes this many photons of ONE batch per visit of the work counter; a lane hands its counts over when
  // its batch changes, so longer chunks mean fewer atomics, shorter ones a shorter end of the launch)
  static const int chunk = (int)std::max(64ll, env_int("I3RC_FUSED_CHUNK", 512));
  A.chunk = chunk;
  if ((int64_t)A.chunk > nPhotons) A.chunk = (int)std::max<int64_t>(64, nPhotons);
  A.nBatches = (unsigned)count;
  A.chunksPerBatch = (unsigned)((nPhotons + A.chunk - 1) / A.chunk);
  A.replicas = R;
  A.blockStride = h->layout.total;
  A.abortFlag = g.abortFlag;
  A.counterBlocks = (double *)g.counterBlocks.p;
  if ((uint64_t)count * R >= ((uint64_t)1 << 31)) return h->fail("fused launch: too many tally blocks");
  const size_t outBytes = (size_t)count * h->layout.total * sizeof(double);
  const int rc = launch_grid<PhiloxBatchStream>(h, L, A, g.stream, count, timeIt, [&](long long, int) -> int {
    *g.abortFlag = 0;
    HIPCHK(h, hipMemsetAsync(g.blocks.p, 0, outBytes * R, g.stream));
    HIPCHK(h, hipMemsetAsync(g.counter.p, 0, sizeof(unsigned long long), g.stream));
    HIPCHK(h, hipMemsetAsync(g.counterBlocks.p, 0, (size_t)count * kCounterReplicas * I3RC_NUM_COUNTERS * sizeof(double), g.stream));
    return 0;
  });
  if (rc) return 1;
  const double *result = (const double *)g.blocks.p;
  if (R > 1) {
    const long long n = (long long)count * h->layout.total;
    hipLaunchKernelGGL(reduce_replicas_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g.stream, (const double *)g.blocks.p,
                       (double *)g.compact.p, (long long)count, R, (long long)h->layout.total);
    HIPCHK(h, hipGetLastError());
    result = (const double *)g.compact.p;
  }
  if (absorbed_columns(h, g.stream, const_cast<double *>(result), count, (long long)h->layout.total)) return 1;
  {
    const long long n = (long long)count * I3RC_NUM_COUNTERS;
    hipLaunchKernelGGL(reduce_counters_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g.stream, (const double *)g.counterBlocks.p,
                       const_cast<double *>(result), (long long)count, (long long)h->layout.total, (int)h->view.counters);
    HIPCHK(h, hipGetLastError());
  }
  if (moments) {
    if (accumulate_moments(h, g.stream, result, count, g.excess)) return 1;
    HIPCHK(h, hipEventRecord(g.done, g.stream));
  } else {
    HIPCHK(h, hipEventRecord(g.traced, g.stream));
    HIPCHK(h, hipStreamWaitEvent(h->fusedCopyStream, g.traced, 0));
    HIPCHK(h, hipMemcpyAsync(g.pinned, result, outBytes, hipMemcpyDeviceToHost, h->fusedCopyStream));
    HIPCHK(h, hipEventRecord(g.done, h->fusedCopyStream));
  }
  g.count = count; g.seed1 = seed1; g.next = 0;
  if (tracing()) std::fprintf(stderr, "[i3rc %9.3f ms] fused group launched: seed words %u .. %u (%d batches of %lld photons, %d replicas, chunk %d)\n", trace_ms(),
                              seed1, seed1 + (unsigned)count - 1u, count, (long long)nPhotons, R, A.chunk);
  return 0;
}

void moments_layout(const i3rc_hip_integrator *h, i3rc_moments_layout &L) {
  const int64_t ncol = (int64_t)h->nx * h->ny, ncell = ncol * h->nz;
  int64_t o = 0;
  L.fluxUp = o; o += ncol; L.fluxDown = o; o += ncol; L.fluxAbsorbed = o; o += ncol;
  L.volumeAbsorption = o; o += ncell;
  L.intensity = o; o += (int64_t)h->nDir * ncol;
  L.absorbedProfile = o; o += h->nz;
  L.meanFluxUp = o++; L.meanFluxDown = o++; L.meanFluxAbsorbed = o++;
  L.meanIntensity = o; o += h->nDir;
  L.total = o;
}

// makes the handle's moment sums ready (zeroed) for a loop of batches -- those of the diagnostic tally too, where one is switched on
int begin_moments(i3rc_hip_integrator *h) {
  i3rc_moments_layout L;
  moments_layout(h, L);
  const size_t bytes = (size_t)L.total * sizeof(double), extraBytes = (size_t)extra_moments_layout(h->extra, h->nx, h->ny, h->nz).total * sizeof(double);
  if (h->momSum.bytes != bytes) { HIPCHK(h, h->momSum.alloc(bytes)); HIPCHK(h, h->momSq.alloc(bytes)); }
  if (h->momExtraSum.bytes != extraBytes) { HIPCHK(h, h->momExtraSum.alloc(extraBytes)); HIPCHK(h, h->momExtraSq.alloc(extraBytes)); }
  if (!h->momCounters.p) HIPCHK(h, h->momCounters.alloc(I3RC_NUM_COUNTERS * sizeof(double)));
  if (!h->momDz.p) {
    HIPCHK(h, h->momDz.upload(h->layerDepth.data(), h->layerDepth.size() * sizeof(double)));
    HIPCHK(h, h->momArea.upload(h->areaFrac.data(), h->areaFrac.size() * sizeof(double)));
  }
  for (DevBuf *m : {&h->momSum, &h->momSq, &h->momExtraSum, &h->momExtraSq, &h->momCounters})
    if (m->p) HIPCHK(h, hipMemset(m->p, 0, m->bytes));
  return 0;
}
// ... and those of the path tally that is switched on (after begin_moments)
int begin_path_moments(i3rc_hip_integrator *h) {
  const size_t bytes = (size_t)path_moments_layout(h->extra, h->nx, h->ny, h->pathBins, (int)h->pathK.size()).total * sizeof(double);
  if (h->momPathSum.bytes != bytes || !h->momPathSum.p) { HIPCHK(h, h->momPathSum.alloc(bytes)); HIPCHK(h, h->momPathSq.alloc(bytes)); }
  for (DevBuf *m : {&h->momPathSum, &h->momPathSq}) HIPCHK(h, hipMemset(m->p, 0, m->bytes));
  return 0;
}

// One moments pass: the fields and means F yields of `count` raw blocks on `stream`, x and x^2 added to `sum` / `sumSq`
template <class Fields>
void launch_moments(hipStream_t stream, const Fields &F, const double *blocks, int count, long long stride, DevBuf &sum, DevBuf &sumSq, double *counterTotals) {
  // (slices of the batch range: enough threads for the chip -- 256 CUs x 8 workgroups -- however few the elements are, at least 8 batches a slice)
  const long long fieldBlocks = (F.fields() + 255) / 256;
  const int slices = (int)std::max<long long>(1, std::min<long long>({(long long)(count + 7) / 8, (2048 + fieldBlocks - 1) / fieldBlocks, 65535}));
  hipLaunchKernelGGL(moments_fields_kernel<Fields>, dim3((unsigned)fieldBlocks, (unsigned)slices), dim3(256), 0, stream, F, blocks, count, stride,
                     (double *)sum.p, (double *)sumSq.p);
  hipLaunchKernelGGL(moments_means_kernel<Fields>, dim3((unsigned)(count * F.means())), dim3(256), 0, stream, F, blocks, stride, (double *)sum.p,
                     (double *)sumSq.p, counterTotals);
}

// `count` raw tally blocks on the device (the handle's layout, counters filled in) -> normalised, x and x^2 added to the
// handle's moment sums, the diagnostic block's (where the layout has one) to those of its own; asynchronous on `stream` (blocks from
// several streams may be added at the same time: float64 atomics)
int accumulate_moments(i3rc_hip_integrator *h, hipStream_t stream, const double *blocks, int count, DevBuf &excess) {
  BatchFields F;
  F.V = current_view(h);
  F.V.areaFrac = (const double *)h->momArea.p; F.V.dz = (const double *)h->momDz.p;
  moments_layout(h, F.L);
  const long long stride = h->layout.total;
  if (F.V.limitContrib) {
    const int per = (h->ncomp + 1) * h->nDir;
    const size_t need = (size_t)count * per * sizeof(double);
    if (excess.bytes < need) HIPCHK(h, excess.alloc(need));
    hipLaunchKernelGGL(moments_excess_kernel, dim3((unsigned)(count * per)), dim3(256), 0, stream, F.V, blocks, stride, (double *)excess.p);
  }
  F.excessSums = (const double *)excess.p;
  launch_moments(stream, F, blocks, count, stride, h->momSum, h->momSq, (double *)h->momCounters.p);
  if (h->extra == EXTRA_LEVELS || h->extra == EXTRA_TRACKS)
    launch_moments(stream, ExtraFields{F.V, h->extra}, blocks, count, stride, h->momExtraSum, h->momExtraSq, nullptr);
  if (h->extra == EXTRA_PATHS || h->extra == EXTRA_PATH_BINS) {   // (i3rc_hip_run_batches_path_moments: no other loop runs with these kinds on)
    // (the edges behind the table's first word, nBins: see i3rc_hip_set_path_histogram)
    const PathFields P{F.V, h->extra, h->pathBins, (int)h->pathK.size(), h->extra == EXTRA_PATH_BINS ? (const float *)h->dBins.p + 1 : nullptr,
                       (const float *)h->dPathK.p};
    // (one slice of the batch range: these kinds come one batch per call, never in a fused group)
    const long long fieldBlocks = (P.fields() + 255) / 256;
    hipLaunchKernelGGL(moments_fields_kernel<PathFields>, dim3((unsigned)fieldBlocks, 1u), dim3(256), 0, stream, P, blocks, count, stride,
                       (double *)h->momPathSum.p, (double *)h->momPathSq.p);
    if (P.quantities() > 0)
      hipLaunchKernelGGL(path_quantities_kernel, dim3((unsigned)(count * P.quantities())), dim3(256), 0, stream, P, blocks, stride,
                         (double *)h->momPathSum.p, (double *)h->momPathSq.p);
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}

// ... and the sums of a finished loop to the caller's arrays (counters, and the diagnostic pair: where the caller wants them)
int download_moments(i3rc_hip_integrator *h, double *sum, double *sumSquares, double *counters, double *extraSum, double *extraSumSquares,
                     double *pathSum = nullptr, double *pathSumSquares = nullptr) {
  const std::pair<double *, const DevBuf *> copies[] = {{sum, &h->momSum}, {sumSquares, &h->momSq}, {counters, &h->momCounters},
                                                         {extraSum, &h->momExtraSum}, {extraSumSquares, &h->momExtraSq},
                                                         {pathSum, &h->momPathSum}, {pathSumSquares, &h->momPathSq}};
  for (const auto &c : copies)
    if (c.first) HIPCHK(h, hipMemcpy(c.first, c.second->p, c.second->bytes, hipMemcpyDeviceToHost));
  return 0;
}

// (hostTallies == nullptr: moments mode -- nothing comes back per batch, see i3rc_hip_run_batches_moments)
int run_batches_fused(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons, const i3rc_source *src,
                      double *hostTallies) {
  const bool moments = hostTallies == nullptr;
  const int G = fused_group_size(h, nBatches, nPhotons, moments);
  const size_t blockBytes = (size_t)h->layout.total * sizeof(double);
  for (auto &g : h->fused) g.count = 0;   // (begin_batch_loop has called the look-ahead off, whose groups held them)
  int rc = 0;
  auto collect = [&](i3rc_hip_integrator::FusedSlot &g) -> int {
    if (g.count == 0) return 0;
    HIPCHK(h, hipEventSynchronize(g.done));
    if (!moments) std::memcpy(hostTallies + (size_t)g.first * (size_t)h->layout.total, g.pinned, (size_t)g.count * blockBytes);
    g.count = 0;
    return 0;
  };
  int k = 0;
  for (int first = 0; first < nBatches && !rc; first += G, ++k) {
    auto &g = h->fused[k % i3rc_hip_integrator::kFusedSlots];
    if ((rc = collect(g))) break;
    const int count = std::min(G, nBatches - first);
    rc = launch_fused_group(h, g, seed0, seed1 + (uint32_t)first, count, nPhotons, src, true, G, moments);
    if (!rc) g.first = first;
  }
  for (int j = 0; j < i3rc_hip_integrator::kFusedSlots; ++j) {   // drain in launch order (also after a failure: nothing stays in flight)
    auto &g = h->fused[(k + j) % i3rc_hip_integrator::kFusedSlots];
    if (rc) { if (g.stream) (void)hipStreamSynchronize(g.stream); g.count = 0; }
    else rc = collect(g);
  }
  return rc;
}


// Launches fused groups ahead of the caller until three are under way: the batches after the last group launched (or from
// `nextIfNone`), 8, 16, 32 ... 256 batches a group -- small groups first, so that the caller's first batches are there soon.
// A loop the caller has announced (i3rc_hip_expect_batches) is never overshot.
void top_up_groups(i3rc_hip_integrator *h, uint32_t seed0, uint32_t nextIfNone, int64_t nPhotons, const i3rc_source *src) {
  while ((int)h->aheadGroups.size() < i3rc_hip_integrator::kFusedSlots) {
    int k = -1;
    for (int j = 0; j < i3rc_hip_integrator::kFusedSlots; ++j) if (h->fused[j].count == 0) { k = j; break; }
    if (k < 0) break;
    uint32_t next = nextIfNone;
    if (!h->aheadGroups.empty()) { const auto &last = h->fused[h->aheadGroups.back()]; next = last.seed1 + (uint32_t)last.count; }
    int want = h->aheadGroupSize <= 0 ? 8 : std::min(256, 2 * h->aheadGroupSize);
    if (h->aheadBounded) {
      const int64_t left = (int64_t)h->aheadEnd - (int64_t)next;
      if (left <= 0) break;
      want = (int)std::min<int64_t>(want, left);
    }
    int size = fused_group_size(h, want, nPhotons);
    // What a slot is made for.  An ANNOUNCED loop: its largest group at once (a slot that grows later waits for the device twice).
    // A loop that is only guessed at (an unchanged driver's calls): at most 96 MiB of pinned memory per slot -- a Landsat-sized
    // field would otherwise hold 3 x (256 MiB pinned + 256 MiB of device memory) per handle for a loop of any length --, and its
    // groups stay within that, so that such a slot never grows either.
    int reserve;
    if (h->aheadBounded) reserve = (int)std::min<int64_t>(fused_group_size(h, 256, nPhotons), (int64_t)h->aheadEnd - (int64_t)next);
    else {
      const int64_t blockBytes = h->layout.total * (int64_t)sizeof(double);
      reserve = (int)std::max<int64_t>(1, std::min<int64_t>(fused_group_size(h, 256, nPhotons), ((int64_t)96 << 20) / blockBytes));
      size = std::min(size, reserve);
    }
    if (launch_fused_group(h, h->fused[k], seed0, next, size, nPhotons, src, false, std::max(reserve, size))) {   // (not the caller's failure)
      h->fused[k].count = 0;
      h->fusedAheadFailed = true;   // (remembered: the caller's loop goes on with single batches launched ahead, see i3rc_hip_compute_batch)
      break;
    }
    h->aheadGroupSize = std::max(h->aheadGroupSize, want);
    h->aheadGroups.push_back(k);
  }
}

// Workgroups keep their partial flux / radiance sums in float32 (LDS): a workgroup must not see so many photons
// that a column's sum could leave the range where float32 still counts (2^24).  Per-photon random streams make a
// long batch the same as several launches over consecutive photon ranges, so very long Directional batches are cut
// into launches of at most 2^22 photons per compute unit (about 1e9 photons on an MI355X).
int launch_extra(i3rc_hip_integrator *h, const Launch &L, const RunArgs &A, hipStream_t stream, bool timeIt);   // (at the end of this file)
int launch_batch_parts(i3rc_hip_integrator *h, const Launch &L, const RunArgs &A, hipStream_t stream, bool timeIt) {
  const int64_t perLaunch = h->launchLimit > 0 ? h->launchLimit : (int64_t)h->numCU << 22;
  // (an extra tally block switched on: the same photons through the general flux kernel under the kind's tag, see launch_extra)
  const auto run = [&](const RunArgs &part) {
    return h->extra == EXTRA_NONE ? launch<PhiloxStream>(h, L, part, stream, timeIt) : launch_extra(h, L, part, stream, timeIt);
  };
  if (A.srcKind != 0) return run(A);
  for (int64_t done = 0; done < A.nPhotons; done += perLaunch) {
    RunArgs part = A;
    part.firstPhoton = A.firstPhoton + done;
    part.nPhotons = std::min<int64_t>(perLaunch, A.nPhotons - done);
    if (run(part)) return 1;
  }
  return 0;
}

// One Directional batch into pipeline slot `sl`: zeroed and traced, asynchronous on the slot's stream.  `who` names the caller in the
// error texts.
int run_batch_in_slot(i3rc_hip_integrator *h, i3rc_hip_integrator::PipeSlot &sl, uint32_t seed0, uint32_t seed1, int64_t nPhotons,
                      const i3rc_source *src, bool timeIt, const char *who) {
  Launch L;
  RunArgs A;
  std::memset(&A, 0, sizeof(A));
  A.seed0 = seed0; A.seed1 = seed1; A.firstPhoton = 0; A.nPhotons = nPhotons;
  A.workCounter = (unsigned long long *)sl.counter.p;
  if (prepare_launch(h, plain_stream(h->extra), src, nPhotons, sl.stream, (double *)sl.tally.p, L, A)) return 1;
  const size_t bytes = (size_t)h->layout.total * sizeof(double);
  if (hipMemsetAsync(sl.tally.p, 0, bytes, sl.stream) != hipSuccess) return h->fail(std::string(who) + ": clearing a tally buffer failed");
  return launch_batch_parts(h, L, A, sl.stream, timeIt);
}
// ... and its block on the way into the slot's pinned buffer behind the trace; sl.done tells when it is there
int copy_back_slot(i3rc_hip_integrator *h, i3rc_hip_integrator::PipeSlot &sl, const char *who) {
  if (hipMemcpyAsync(sl.pinned, sl.tally.p, (size_t)h->layout.total * sizeof(double), hipMemcpyDeviceToHost, sl.stream) != hipSuccess ||
      hipEventRecord(sl.done, sl.stream) != hipSuccess)
    return h->fail(std::string(who) + ": copying a batch's tallies back failed");
  return 0;
}

// What the three calls that run a driver's loop do first, `who` in the error texts: the checks (argsOk: the caller's pointers and
// batch count), then the handle made ready -- the look-ahead called off (i3rc_hip_compute_batch shares the slots), and whatever the
// caller had in flight on the handle's stream comes first.  diagnostic: the loop is one WITH a diagnostic tally, which must be on and
// fit a plain launch (the call then names itself in front of the photon count's text too); any other loop has none.
// paths: the loop is one with a path tally (i3rc_hip_run_batches_path_moments), which must be on likewise.
int begin_batch_loop(i3rc_hip_integrator *h, const std::string &who, bool argsOk, const i3rc_source *src, int64_t nPhotons, bool diagnostic,
                     bool paths = false) {
  if (!h) return 1;
  if (!argsOk) return h->fail(who + ": bad arguments");
  if (paths) {
    if (h->extra == EXTRA_RADIANCE_PATHS) return h->fail(who + ": " + no_radiance_path_moments_text());
    if (h->extra != EXTRA_PATHS && h->extra != EXTRA_PATH_BINS)
      return h->fail(who + ": no path tally is switched on (i3rc_hip_set_path_lengths or i3rc_hip_set_path_histogram first; "
                     "i3rc_hip_run_batches_diagnostic_moments serves the other diagnostic tallies)");
    diagnostic = false;   // (nor does the diagnostic moments' refusal of these kinds apply)
  }
  if (diagnostic && h->extra == EXTRA_NONE)
    return h->fail(who + ": no diagnostic tally is switched on (i3rc_hip_set_level_fluxes or i3rc_hip_set_actinic_flux first; "
                   "i3rc_hip_run_batches_moments serves a loop without one)");
  if (diagnostic && h->extra == EXTRA_PATHS) return h->fail(who + ": " + no_path_moments_text());
  if (diagnostic && h->extra == EXTRA_PATH_BINS) return h->fail(who + ": " + no_bin_moments_text());
  if (h->extra == EXTRA_RADIANCE_PATHS) return h->fail(who + ": " + no_radiance_path_moments_text());   // (every loop: fused, moments, diagnostic)
  if (src->kind != 0) return h->fail(who + ": Directional photon streams only (explicit streams differ from batch to batch)");
  if (nPhotons <= 0) return h->fail((diagnostic || paths ? who + ": " : "") + "setIllumination: must ask for non-negative number of photons.");
  if (extra_tally_refused(h, who.c_str(), !diagnostic && !paths)) return 1;
  HIPCHK(h, hipSetDevice(h->device));
  drop_lookahead(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

// A loop's batches one launch each, batch b into slot b % K, up to K in flight (inFlight <= 0: six): behind a batch's trace
// `queue(slot)` puts the call's own work on the slot's stream, and `finish(slot)` waits for a batch and takes what the call wants of
// it -- before its slot is used again, and for every slot at the end.  Nothing of the call stays in flight, also after a failure.
template <class Queue, class Finish>
int run_batch_pipeline(i3rc_hip_integrator *h, const char *who, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons, const i3rc_source *src,
                       int inFlight, Queue &&queue, Finish &&finish) {
  const int K = std::min(nBatches, inFlight <= 0 ? 6 : std::min(inFlight, (int)i3rc_hip_integrator::kMaxInFlight));
  if (reset_slots_if_layout_changed(h)) return 1;
  for (int k = 0; k < K; ++k) {
    if (ready_slot(h, k)) return 1;
    h->pipe[k].batch = -1;
  }
  int rc = 0;
  for (int b = 0; b < nBatches && !rc; ++b) {
    auto &sl = h->pipe[b % K];
    if (sl.batch >= 0) rc = finish(sl);
    rc = rc || run_batch_in_slot(h, sl, seed0, seed1 + (uint32_t)b, nPhotons, src, true, who) || queue(sl);
    if (!rc) sl.batch = b;
  }
  for (int k = 0; k < K; ++k) {
    auto &sl = h->pipe[k];
    if (!rc && sl.batch >= 0) rc = finish(sl);
    if (rc) (void)hipStreamSynchronize(sl.stream);
    sl.batch = -1;
  }
  return rc;
}

}  // namespace

extern "C" {

int i3rc_hip_launch_batch(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int64_t firstPhoton, int64_t nPhotons,
                          const i3rc_source *src) {
  if (!h) return 1;
  if (!src) return h->fail("i3rc_hip_launch_batch: null source");
  if (nPhotons <= 0) return h->fail("setIllumination: must ask for non-negative number of photons.");  // illumination :78-79
  if (extra_tally_refused(h, "i3rc_hip_launch_batch", false)) return 1;
  HIPCHK(h, hipSetDevice(h->device));
  Launch L;
  RunArgs A;
  std::memset(&A, 0, sizeof(A));
  A.seed0 = seed0; A.seed1 = seed1; A.firstPhoton = firstPhoton; A.nPhotons = nPhotons;
  A.workCounter = (unsigned long long *)h->workCounter.p;
  if (prepare_launch(h, plain_stream(h->extra), src, nPhotons, h->stream, h->tally, L, A)) return 1;
  return launch_batch_parts(h, L, A, h->stream, true);
}

// The batch loop of a driver (Example-Drivers/monteCarloDriver.f95:283-326) as one call: see include/i3rc_hip.h
int i3rc_hip_run_batches(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons,
                         const i3rc_source *src, int inFlight, double *hostTallies) {
  static const char who[] = "i3rc_hip_run_batches";
  if (begin_batch_loop(h, who, src && hostTallies && nBatches >= 1, src, nPhotons, false)) return 1;
  if (fuse_loop(h, nPhotons, nBatches)) return run_batches_fused(h, seed0, seed1, nBatches, nPhotons, src, hostTallies);
  // every batch's block comes back through its slot's pinned buffer
  return run_batch_pipeline(
      h, who, seed0, seed1, nBatches, nPhotons, src, inFlight, [&](i3rc_hip_integrator::PipeSlot &sl) { return copy_back_slot(h, sl, who); },
      [&](i3rc_hip_integrator::PipeSlot &sl) -> int {
        HIPCHK(h, hipEventSynchronize(sl.done));
        std::memcpy(hostTallies + (size_t)sl.batch * (size_t)h->layout.total, sl.pinned, (size_t)h->layout.total * sizeof(double));
        return 0;
      });
}

int i3rc_hip_get_moments_layout(const i3rc_hip_integrator *h, i3rc_moments_layout *layout) {
  if (!h || !layout) return 1;
  moments_layout(h, *layout);
  return 0;
}

// A loop's batches with their statistics gathered on the device (the two entry points below; extraSum / extraSumSquares: the
// diagnostic tally's, nullptr for a loop without one).  Problems whose batches share a grid go there group by group; the others (the
// general kernels -- a diagnostic tally's among them --, long batches) one launch per batch, each batch's block normalised and added up
// on its slot's stream behind its trace.
static int run_batches_moments(i3rc_hip_integrator *h, const char *who, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons,
                               const i3rc_source *src, double *sum, double *sumSquares, double *counters, double *extraSum, double *extraSumSquares,
                               double *pathSum = nullptr, double *pathSumSquares = nullptr) {
  if (begin_moments(h) || (pathSum && begin_path_moments(h))) return 1;
  const int rc =
      h->extra == EXTRA_NONE && fuse_loop(h, nPhotons, nBatches)   // (no fused kernel fills a diagnostic block: extra_tally_refused)
          ? run_batches_fused(h, seed0, seed1, nBatches, nPhotons, src, nullptr)
          : run_batch_pipeline(
                h, who, seed0, seed1, nBatches, nPhotons, src, 0,
                [&](i3rc_hip_integrator::PipeSlot &sl) { return accumulate_moments(h, sl.stream, (const double *)sl.tally.p, 1, sl.excess); },
                [&](i3rc_hip_integrator::PipeSlot &sl) {
                  return hipStreamSynchronize(sl.stream) == hipSuccess ? 0 : h->fail(std::string(who) + ": waiting for the batches failed");
                });
  return rc || download_moments(h, sum, sumSquares, counters, extraSum, extraSumSquares, pathSum, pathSumSquares);
}

int i3rc_hip_run_batches_moments(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons,
                                 const i3rc_source *src, double *sum, double *sumSquares, double *counters) {
  static const char who[] = "i3rc_hip_run_batches_moments";
  return begin_batch_loop(h, who, src && sum && sumSquares && nBatches >= 1, src, nPhotons, false) ||
         run_batches_moments(h, who, seed0, seed1, nBatches, nPhotons, src, sum, sumSquares, counters, nullptr, nullptr);
}

int i3rc_hip_diagnostic_moments_layout_words(int kind, int nx, int ny, int nz, int64_t *out, int nout) {
  if (kind < EXTRA_NONE || kind > EXTRA_TRACKS || nx < 1 || ny < 1 || nz < 1 || !out || nout < 7) return 1;
  const ExtraMomentsLayout L = extra_moments_layout((ExtraTally)kind, nx, ny, nz);
  const int64_t v[7] = {L.levelFluxUp, L.levelFluxDown, L.meanLevelFluxUp, L.meanLevelFluxDown, L.actinicFlux, L.meanActinicFlux, L.total};
  for (int k = 0; k < 7; ++k) out[k] = v[k];
  return 0;
}

int i3rc_hip_get_diagnostic_moments_layout(const i3rc_hip_integrator *h, i3rc_diagnostic_moments_layout *layout) {
  if (!h || !layout) return 1;
  if (h->extra == EXTRA_PATHS) return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_get_diagnostic_moments_layout: " + no_path_moments_text());
  if (h->extra == EXTRA_PATH_BINS) return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_get_diagnostic_moments_layout: " + no_bin_moments_text());
  if (h->extra == EXTRA_RADIANCE_PATHS)
    return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_get_diagnostic_moments_layout: " + no_radiance_path_moments_text());
  const ExtraMomentsLayout L = extra_moments_layout(h->extra, h->nx, h->ny, h->nz);
  layout->kind = (int64_t)h->extra;
  layout->levelFluxUp = L.levelFluxUp; layout->levelFluxDown = L.levelFluxDown; layout->meanLevelFluxUp = L.meanLevelFluxUp;
  layout->meanLevelFluxDown = L.meanLevelFluxDown; layout->actinicFlux = L.actinicFlux; layout->meanActinicFlux = L.meanActinicFlux;
  layout->total = L.total;
  return 0;
}

// A driver's batch loop with a diagnostic tally switched on, its statistics gathered on the device: see include/i3rc_hip.h
int i3rc_hip_run_batches_diagnostic_moments(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons,
                                            const i3rc_source *src, double *sum, double *sumSquares, double *counters, double *extraSum,
                                            double *extraSumSquares) {
  static const char who[] = "i3rc_hip_run_batches_diagnostic_moments";
  return begin_batch_loop(h, who, src && sum && sumSquares && extraSum && extraSumSquares && nBatches >= 1, src, nPhotons, true) ||
         run_batches_moments(h, who, seed0, seed1, nBatches, nPhotons, src, sum, sumSquares, counters, extraSum, extraSumSquares);
}

int i3rc_hip_path_moments_layout_words(int kind, int nx, int ny, int nBins, int nK, int64_t *out, int nout) {
  if ((kind != EXTRA_PATHS && kind != EXTRA_PATH_BINS) || nx < 1 || ny < 1 || nK < 0 || nK > kMaxPathSpectrum || !out || nout < kPathMomentsWords) return 1;
  if (kind == EXTRA_PATH_BINS && (nBins < 1 || nBins > kMaxPathBins)) return 1;
  const PathMomentsLayout L = path_moments_layout((ExtraTally)kind, nx, ny, nBins, nK);
  const int64_t v[kPathMomentsWords] = {L.pathLengthUp, L.pathLengthSquaredUp, L.pathLengthDown, L.pathLengthSquaredDown,
                                        L.meanPathLengthUp, L.meanPathLengthSquaredUp, L.meanPathLengthDown, L.meanPathLengthSquaredDown,
                                        L.domainPathUp, L.domainPathSquaredUp, L.domainPathDown, L.domainPathSquaredDown,
                                        L.histogramUp, L.histogramPathUp, L.histogramDown, L.histogramPathDown,
                                        L.spectrumUpLower, L.spectrumUpUpper, L.spectrumDownLower, L.spectrumDownUpper, L.total};
  for (int k = 0; k < kPathMomentsWords; ++k) out[k] = v[k];
  return 0;
}

int i3rc_hip_get_path_moments_layout(const i3rc_hip_integrator *h, i3rc_path_moments_layout *layout) {
  if (!h || !layout) return 1;
  if (h->extra == EXTRA_RADIANCE_PATHS)
    return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_get_path_moments_layout: " + no_radiance_path_moments_text());
  if (h->extra != EXTRA_PATHS && h->extra != EXTRA_PATH_BINS)
    return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_get_path_moments_layout: no path tally is switched on");
  layout->kind = (int64_t)h->extra;
  layout->nBins = h->extra == EXTRA_PATH_BINS ? h->pathBins : 0;
  layout->nK = (int64_t)h->pathK.size();
  // (the struct's offsets are the words of i3rc_hip_path_moments_layout_words, in order)
  return i3rc_hip_path_moments_layout_words((int)h->extra, h->nx, h->ny, h->pathBins, (int)h->pathK.size(), &layout->pathLengthUp, kPathMomentsWords);
}

int i3rc_hip_set_path_spectrum(i3rc_hip_integrator *h, int nK, const float *absorption) {
  if (!h) return 1;
  const std::string who = "i3rc_hip_set_path_spectrum: ";
  if (nK < 0 || nK > kMaxPathSpectrum)
    return h->fail(who + "0 <= nK <= " + std::to_string(kMaxPathSpectrum) + " required (0 switches the spectrum off); got " + std::to_string(nK));
  if (nK > 0 && !absorption) return h->fail(who + "null absorption coefficients (nK float32 values)");
  for (int j = 0; j < nK; ++j) {
    if (!std::isfinite(absorption[j])) return h->fail(who + "absorption coefficients must be finite; absorption[" + std::to_string(j) + "] is not");
    if (absorption[j] < 0.0f) return h->fail(who + "absorption coefficients must not be negative; absorption[" + std::to_string(j) + "] is");
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (nK > 0) {
    const hipError_t e = h->dPathK.upload(absorption, sizeof(float) * (size_t)nK);
    if (e != hipSuccess) { h->pathK.clear(); return h->hipfail("i3rc_hip_set_path_spectrum: uploading the absorption coefficients", e); }
  }
  h->pathK.assign(absorption, absorption + nK);
  return 0;
}

// A driver's batch loop with a path tally switched on, its statistics gathered on the device: see include/i3rc_hip.h
int i3rc_hip_run_batches_path_moments(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons, const i3rc_source *src,
                                      double *sum, double *sumSquares, double *counters, double *pathSum, double *pathSumSquares) {
  static const char who[] = "i3rc_hip_run_batches_path_moments";
  return begin_batch_loop(h, who, src && sum && sumSquares && pathSum && pathSumSquares && nBatches >= 1, src, nPhotons, false, true) ||
         run_batches_moments(h, who, seed0, seed1, nBatches, nPhotons, src, sum, sumSquares, counters, nullptr, nullptr, pathSum, pathSumSquares);
}

// computeRadiativeTransfer for one batch of a driver's loop, looking ahead: see include/i3rc_hip.h
int i3rc_hip_compute_batch(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int64_t nPhotons, const i3rc_source *src,
                           int lookAhead, double *hostTallies) {
  if (!h) return 1;
  if (!src || !hostTallies) return h->fail("i3rc_hip_compute_batch: bad arguments");
  if (src->kind != 0) return h->fail("i3rc_hip_compute_batch: Directional photon streams only");
  if (nPhotons <= 0) return h->fail("setIllumination: must ask for non-negative number of photons.");
  if (extra_tally_refused(h, "i3rc_hip_compute_batch", false)) return 1;
  HIPCHK(h, hipSetDevice(h->device));
  // (an extra tally block switched on: no look-ahead -- one launch per call)
  const int depth = h->extra != EXTRA_NONE ? 0 : std::max(0, std::min(lookAhead, (int)i3rc_hip_integrator::kMaxInFlight - 1));
  const size_t bytes = (size_t)h->layout.total * sizeof(double);
  if (reset_slots_if_layout_changed(h)) return 1;   // (a change of the layout has dropped the queue already: set_directions)
  auto free_slot = [&]() -> int {
    for (int k = 0; k < i3rc_hip_integrator::kMaxInFlight; ++k) if (h->pipe[k].batch < 0) return k;
    return -1;
  };
  auto start = [&](int k, uint32_t s1, bool timed) -> int {   // (batches launched ahead of the caller are not recorded in the ring of timed launches)
    static const char who[] = "i3rc_hip_compute_batch";
    if (ready_slot(h, k) || run_batch_in_slot(h, h->pipe[k], seed0, s1, nPhotons, src, timed, who) || copy_back_slot(h, h->pipe[k], who)) return 1;
    h->pipe[k].batch = 0;   // in use (any value >= 0; i3rc_hip_run_batches keeps a batch number here)
    return 0;
  };
  i3rc_hip_integrator::BatchSignature sig;
  sig.seed0 = seed0; sig.n = nPhotons; sig.mu = src->solarMu; sig.az = src->solarAzimuth; sig.set = true;
  // Problems whose batches can share a grid (fuse_loop) are looked ahead in GROUPS: 8, 16, 32 ... 256 batches per fused
  // launch, up to three groups under way (one after the other on the device), the caller served from the oldest.  Such launches are not timed (the ring of
  // i3rc_hip_kernel_ms_history holds launches the caller asked for), and a group that is not wanted after all is called
  // off through its abort word: its waves stop at their next visit of the work counter.
  const bool fuse = depth > 0 && fuse_loop(h, nPhotons, 2);   // (a loop of unknown length: fused as any loop of several batches)
  // (a group that could not be launched -- memory -- is not tried again at every call: groups under way are still handed out)
  auto top_up = [&]() { if (!h->fusedAheadFailed) top_up_groups(h, seed0, seed1 + 1u, nPhotons, src); };
  if (!h->aheadGroups.empty()) {
    auto &g = h->fused[h->aheadGroups.front()];
    if (fuse && h->aheadSig == sig && g.seed1 + (uint32_t)g.next == seed1) {
      const double tw = tracing() ? trace_ms() : 0.0;
      if (hipEventSynchronize(g.done) != hipSuccess) { drop_lookahead(h); return h->fail("i3rc_hip_compute_batch: waiting for the batch failed"); }
      if (tracing() && trace_ms() - tw > 0.5) std::fprintf(stderr, "[i3rc %9.3f ms] batch %u waited %.3f ms for its group\n", trace_ms(), seed1, trace_ms() - tw);
      std::memcpy(hostTallies, g.pinned + (size_t)g.next * (size_t)h->layout.total, bytes);
      if (++g.next == g.count) { g.count = 0; h->aheadGroups.erase(h->aheadGroups.begin()); }
      h->lastSig = sig; h->lastSeed1 = seed1;
      top_up();
      if (h->aheadBounded && h->aheadGroups.empty()) h->aheadBounded = false;   // the announced loop is through: from here on the usual guessing
      return 0;
    }
    drop_lookahead(h);
  }
  // batches launched ahead serve this call only if the next of them is exactly this batch
  if (!h->aheadQueue.empty() && !(h->aheadSig == sig && h->aheadQueue.front().seed1 == seed1)) drop_lookahead(h);
  int mine;
  if (!h->aheadQueue.empty()) {
    mine = h->aheadQueue.front().slot;
    h->aheadQueue.erase(h->aheadQueue.begin());
  } else {
    mine = free_slot();
    if (mine < 0) return h->fail("i3rc_hip_compute_batch: no free slot");
    if (start(mine, seed1, true)) { drop_lookahead(h); return 1; }
  }
  h->pipe[mine].batch = 0;   // (in use until its tallies have been handed over)
  // look ahead once the caller's loop shows: the same batch as last time with the next seed word (monteCarloDriver.f95:277)
  const bool inLoop = h->lastSig == sig && h->lastSeed1 + 1u == seed1;
  h->lastSig = sig; h->lastSeed1 = seed1;
  if (fuse && inLoop) {
    h->aheadSig = sig;
    top_up();
  }
  if (!(fuse && inLoop && !h->aheadGroups.empty()) && depth > 0 && (inLoop || !h->aheadQueue.empty())) {   // (also when no fused group could be launched)
    h->aheadSig = sig;
    while ((int)h->aheadQueue.size() < depth) {
      const uint32_t next = (h->aheadQueue.empty() ? seed1 : h->aheadQueue.back().seed1) + 1u;
      const int k = free_slot();
      if (k < 0 || start(k, next, false)) break;   // (a failed look-ahead is not this batch's failure: the error text stays for the next call)
      h->aheadQueue.push_back({next, k});
    }
  }
  auto &sl = h->pipe[mine];
  if (hipEventSynchronize(sl.done) != hipSuccess) { drop_lookahead(h); sl.batch = -1; return h->fail("i3rc_hip_compute_batch: waiting for the batch failed"); }
  std::memcpy(hostTallies, sl.pinned, bytes);
  sl.batch = -1;
  return 0;
}

// Announces a driver's loop to i3rc_hip_compute_batch: see include/i3rc_hip.h
int i3rc_hip_expect_batches(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int nBatches, int64_t nPhotons, const i3rc_source *src,
                            int *accepted) {
  if (!h) return 1;
  if (accepted) *accepted = 0;
  if (!src || nBatches < 1) return h->fail("i3rc_hip_expect_batches: bad arguments");
  if (src->kind != 0) return h->fail("i3rc_hip_expect_batches: Directional photon streams only");
  if (nPhotons <= 0) return h->fail("setIllumination: must ask for non-negative number of photons.");
  if (extra_tally_refused(h, "i3rc_hip_expect_batches", true)) return 1;
  HIPCHK(h, hipSetDevice(h->device));
  drop_lookahead(h);
  if (!fuse_loop(h, nPhotons, nBatches)) return 0;   // (the caller goes on as it would have)
  {   // the problem must be complete before anything is launched (as i3rc_hip_compute_batch would find out)
    if (const char *missing = incomplete(*h)) return h->fail(missing);
  }
  i3rc_hip_integrator::BatchSignature sig;
  sig.seed0 = seed0; sig.n = nPhotons; sig.mu = src->solarMu; sig.az = src->solarAzimuth; sig.set = true;
  h->aheadSig = sig;
  h->lastSig = sig; h->lastSeed1 = seed1 - 1u;
  h->aheadBounded = true; h->aheadEnd = seed1 + (uint32_t)nBatches;
  h->aheadGroupSize = 16;   // (the first group: 32 batches)
  top_up_groups(h, seed0, seed1, nPhotons, src);
  // (the first group could not be launched -- the slot's pinned or device reserve, say: launch_fused_group has left the reason in
  // i3rc_hip_last_error --: not accepted, and the caller goes on with i3rc_hip_run_batches, as the header promises)
  if (h->aheadGroups.empty()) { drop_lookahead(h); return 0; }
  if (accepted) *accepted = 1;
  return 0;
}

int i3rc_hip_run_replay(i3rc_hip_integrator *h, int64_t nPhotons, const i3rc_source *src, const float *randoms,
                        int64_t nRandoms, const int64_t *drawStart, int32_t *fate, int32_t *fateColumn, float *fateWeight,
                        int32_t *fateOrder, int32_t *drawsUsed) {
  if (!h) return 1;
  if (!src || !randoms || !drawStart || nPhotons <= 0) return h->fail("i3rc_hip_run_replay: bad arguments");
  if (h->extra == EXTRA_TRACKS || h->extra == EXTRA_PATHS || h->extra == EXTRA_PATH_BINS || h->extra == EXTRA_RADIANCE_PATHS) {
    const ExtraWords &w = kExtraWords[h->extra];
    return h->fail(std::string("i3rc_hip_run_replay: ") + w.noun + " " + w.are + " tallied by the production stream's kernels only; the replay build has no such kernel (switch " +
                   w.them + " off)");
  }
  HIPCHK(h, hipSetDevice(h->device));
  Launch L;
  RunArgs A;
  std::memset(&A, 0, sizeof(A));
  A.nPhotons = nPhotons;
  A.workCounter = (unsigned long long *)h->workCounter.p;
  if (prepare_launch(h, stream_of<ReplayStream>(), src, nPhotons, h->stream, h->tally, L, A)) return 1;
  DevBuf dR, dS, dFate, dCol, dW, dOrd, dUsed;
  HIPCHK(h, dR.upload(randoms, sizeof(float) * (size_t)nRandoms));
  HIPCHK(h, dS.upload(drawStart, sizeof(int64_t) * (size_t)nPhotons));
  A.randoms = (const float *)dR.p; A.nRandoms = nRandoms; A.drawStart = (const long long *)dS.p;
  const bool rec = fate && fateColumn && fateWeight && fateOrder && drawsUsed;
  if (rec) {
    HIPCHK(h, dFate.alloc(sizeof(int32_t) * nPhotons)); HIPCHK(h, dCol.alloc(sizeof(int32_t) * nPhotons));
    HIPCHK(h, dW.alloc(sizeof(float) * nPhotons)); HIPCHK(h, dOrd.alloc(sizeof(int32_t) * nPhotons));
    HIPCHK(h, dUsed.alloc(sizeof(int32_t) * nPhotons));
    A.fate = (int32_t *)dFate.p; A.fateColumn = (int32_t *)dCol.p; A.fateWeight = (float *)dW.p;
    A.fateOrder = (int32_t *)dOrd.p; A.drawsUsed = (int32_t *)dUsed.p;
  }
  if (launch<ReplayStream>(h, L, A, h->stream, false)) return 1;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (rec) {
    HIPCHK(h, hipMemcpy(fate, dFate.p, sizeof(int32_t) * nPhotons, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(fateColumn, dCol.p, sizeof(int32_t) * nPhotons, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(fateWeight, dW.p, sizeof(float) * nPhotons, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(fateOrder, dOrd.p, sizeof(int32_t) * nPhotons, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(drawsUsed, dUsed.p, sizeof(int32_t) * nPhotons, hipMemcpyDeviceToHost));
  }
  return 0;
}

int i3rc_hip_trace_rays(i3rc_hip_integrator *h, int64_t n, const float *dir, float *pos, int32_t *idx, const float *target,
                        float *tau, int32_t *steps) {
  if (!h) return 1;
  if (n <= 0 || !dir || !pos || !idx || !target || !tau || !steps) return h->fail("i3rc_hip_trace_rays: bad arguments");
  for (int64_t i = 0; i < n; ++i) {  // shapes must match what the kernel indexes
    if (idx[3 * i] < 1 || idx[3 * i] > h->nx || idx[3 * i + 1] < 1 || idx[3 * i + 1] > h->ny || idx[3 * i + 2] < 1 ||
        idx[3 * i + 2] > h->nz)
      return h->fail("i3rc_hip_trace_rays: start cell outside the domain");
  }
  HIPCHK(h, hipSetDevice(h->device));
  // tables are not needed for bare tracing: the geometry and the field alone, in every packed form.  The hook reads the bricked copy
  // (its index is checked bit for bit) unless i3rc_hip_select_grid_place asked for the plain field or the column records
  DevProblem P;
  fill_geometry(h, P);
  const int hookPlace = h->gridPlace == I3RC_GRID_LINEAR ? GRID_GLOBAL : (h->gridPlace == I3RC_GRID_COLUMNS ? (h->colBase ? GRID_COLBASE : GRID_COLUMNS) : GRID_BRICKS);
  DevBuf dDir, dPos, dIdx, dTar, dTau, dSteps;
  HIPCHK(h, dDir.upload(dir, sizeof(float) * 3 * n)); HIPCHK(h, dPos.upload(pos, sizeof(float) * 3 * n));
  HIPCHK(h, dIdx.upload(idx, sizeof(int32_t) * 3 * n)); HIPCHK(h, dTar.upload(target, sizeof(float) * n));
  HIPCHK(h, dTau.alloc(sizeof(float) * n)); HIPCHK(h, dSteps.alloc(sizeof(int32_t) * n));
  const size_t lds = sizeof(float) * ((h->nx + 1) + (h->ny + 1) + (h->nz + 1)) + sizeof(uint32_t) * std::max((size_t)h->clearWords, (size_t)h->nz);
  if (lds > kLdsBudget) return h->fail("i3rc_hip_trace_rays: domain edge vectors do not fit in LDS");
  // (more than 65534 layers: the clear-air map's 16-bit layer numbers do not reach the top -- the hook reads the bricks without it)
  auto *const hook = hookPlace == GRID_GLOBAL ? trace_rays_kernel<GRID_GLOBAL, false>
                   : (hookPlace == GRID_COLUMNS ? trace_rays_kernel<GRID_COLUMNS, false> : hookPlace == GRID_COLBASE ? trace_rays_kernel<GRID_COLBASE, false>
                                                : (h->nz <= 65534 ? trace_rays_kernel<GRID_BRICKS, true> : trace_rays_kernel<GRID_BRICKS, false>));
  hipLaunchKernelGGL(hook, dim3((unsigned)((n + 255) / 256)), dim3(256), lds, h->stream, P, (long long)n,
                     (const float *)dDir.p, (float *)dPos.p, (int32_t *)dIdx.p, (const float *)dTar.p, (float *)dTau.p,
                     (int32_t *)dSteps.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(pos, dPos.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(idx, dIdx.p, sizeof(int32_t) * 3 * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(tau, dTau.p, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(steps, dSteps.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return 0;
}

/* Test hook: raw Philox blocks and the float deviates derived from them, as photon streams see them. */
int i3rc_hip_philox_blocks(i3rc_hip_integrator *h, uint32_t seed0, uint32_t seed1, int64_t firstPhoton, int64_t n,
                           int blocksPerPhoton, uint32_t *out, float *outf) {
  if (!h) return 1;
  if (n <= 0 || blocksPerPhoton <= 0 || !out || !outf) return h->fail("i3rc_hip_philox_blocks: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf d, df;
  const size_t cnt = (size_t)n * blocksPerPhoton * 4;
  HIPCHK(h, d.alloc(cnt * 4)); HIPCHK(h, df.alloc(cnt * 4));
  hipLaunchKernelGGL(philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, seed0, seed1,
                     (long long)firstPhoton, (long long)n, blocksPerPhoton, (uint32_t *)d.p, (float *)df.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, d.p, cnt * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(outf, df.p, cnt * 4, hipMemcpyDeviceToHost));
  return 0;
}

/* Test hook: counts, over n pairs, where the kernel's exact_div / exact_sqrt differ from IEEE `/` and sqrtf. */
int i3rc_hip_arith_check(i3rc_hip_integrator *h, int64_t n, const float *num, const float *den, int64_t *divMismatch,
                         int64_t *sqrtMismatch) {
  if (!h) return 1;
  if (n <= 0 || !num || !den || !divMismatch || !sqrtMismatch) return h->fail("i3rc_hip_arith_check: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf dn, dd, dc;
  HIPCHK(h, dn.upload(num, sizeof(float) * n)); HIPCHK(h, dd.upload(den, sizeof(float) * n));
  HIPCHK(h, dc.alloc(2 * sizeof(unsigned long long)));
  HIPCHK(h, hipMemset(dc.p, 0, 2 * sizeof(unsigned long long)));
  hipLaunchKernelGGL(arith_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (long long)n,
                     (const float *)dn.p, (const float *)dd.p, (unsigned long long *)dc.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned long long c[2];
  HIPCHK(h, hipMemcpy(c, dc.p, sizeof(c), hipMemcpyDeviceToHost));
  *divMismatch = (int64_t)c[0]; *sqrtMismatch = (int64_t)c[1];
  return 0;
}

/* Test hook: findIndex (Code/numericUtilities.f95:195-248) on the device, as the kernels evaluate it. */
int i3rc_hip_find_index(i3rc_hip_integrator *h, int n, const float *table, int64_t m, const float *values, const int32_t *firstGuess,
                        int32_t *out) {
  if (!h) return 1;
  if (n < 1 || m < 1 || !table || !values || !out) return h->fail("i3rc_hip_find_index: bad arguments");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf dt, dv, dg, dout;
  HIPCHK(h, dt.upload(table, sizeof(float) * (size_t)n)); HIPCHK(h, dv.upload(values, sizeof(float) * (size_t)m));
  if (firstGuess) HIPCHK(h, dg.upload(firstGuess, sizeof(int32_t) * (size_t)m));
  HIPCHK(h, dout.alloc(sizeof(int32_t) * (size_t)m));
  hipLaunchKernelGGL(find_index_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, n, (const float *)dt.p, (long long)m,
                     (const float *)dv.p, firstGuess ? (const int32_t *)dg.p : nullptr, (int32_t *)dout.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, dout.p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
  return 0;
}

/* Test hook: computeSurfaceReflectance (Code/surfaceProperties.f95:121-162) on the device for the surface of i3rc_hip_set_surface. */
int i3rc_hip_surface_reflectance(i3rc_hip_integrator *h, int64_t m, const float *x, const float *y, float *out) {
  if (!h) return 1;
  if (m < 1 || !x || !y || !out) return h->fail("i3rc_hip_surface_reflectance: bad arguments");
  if (!h->dBrdf.p) return h->fail("i3rc_hip_surface_reflectance: no surface description set");
  HIPCHK(h, hipSetDevice(h->device));
  DevBuf dx, dy, dout;
  HIPCHK(h, dx.upload(x, sizeof(float) * (size_t)m)); HIPCHK(h, dy.upload(y, sizeof(float) * (size_t)m));
  HIPCHK(h, dout.alloc(sizeof(float) * (size_t)m));
  SurfaceOnly S;
  S.xsE = (const float *)h->dXs.p; S.ysE = (const float *)h->dYs.p; S.brdf = (const float *)h->dBrdf.p; S.nxs = h->nxs; S.nys = h->nys;
  hipLaunchKernelGGL(surface_reflectance_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, S, (long long)m,
                     (const float *)dx.p, (const float *)dy.p, (float *)dout.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, dout.p, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
  return 0;
}

int i3rc_hip_synchronize(i3rc_hip_integrator *h) {
  if (!h) return 1;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int i3rc_hip_fetch_tallies(i3rc_hip_integrator *h, double *host) {
  if (!h) return 1;
  if (!host) return h->fail("i3rc_hip_fetch_tallies: null buffer");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(host, h->tally, (size_t)h->layout.total * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int i3rc_hip_kernel_ms_history(i3rc_hip_integrator *h, int n, float *ms) {
  if (!h || !ms || n < 1) return 1;
  if (n > i3rc_hip_integrator::kEventRing || n > h->timedLaunches)
    return h->fail("i3rc_hip_kernel_ms_history: fewer timed launches recorded than requested (ring of 64)");
  HIPCHK(h, hipSetDevice(h->device));
  for (int k = 0; k < n; ++k) {  // ms[0] = oldest of the last n launches
    const int slot = (int)((h->timedLaunches - n + k) % i3rc_hip_integrator::kEventRing);
    HIPCHK(h, hipEventSynchronize(h->evStop[slot]));
    HIPCHK(h, hipEventElapsedTime(&ms[k], h->evStart[slot], h->evStop[slot]));
  }
  return 0;
}

int i3rc_hip_last_kernel_ms(i3rc_hip_integrator *h, float *ms) { return i3rc_hip_kernel_ms_history(h, 1, ms); }

int64_t i3rc_hip_timed_launch_count(const i3rc_hip_integrator *h) { return h ? (int64_t)h->timedLaunches : 0; }

const char *i3rc_hip_last_kernel_name(const i3rc_hip_integrator *h) { return h ? h->lastKernelName.c_str() : ""; }

int i3rc_hip_last_plan(const i3rc_hip_integrator *h, int32_t *out, int n) {
  if (!h || !out) return 1;
  for (int k = 0; k < std::min(n, kPlanWords); ++k) out[k] = h->lastPlan[k];
  if (n > kPlanBinWord) out[kPlanBinWord] = h->lastPlanBins;
  return 0;
}

int i3rc_hip_normalise(const i3rc_hip_integrator *h, const double *t, float *fluxUp, float *fluxDown, float *fluxAbsorbed,
                       float *volumeAbsorption, float *intensity, float *intensityByComponent) {
  if (!h || !t) return 1;
  const TallyView V = current_view(h);
  const size_t ncol = (size_t)h->nx * h->ny;
  const int nDir = h->nDir, ncomp = h->ncomp;
  for (size_t k = 0; k < ncol; ++k) {
    if (fluxUp) fluxUp[k] = normalised_column_flux(V, t, V.fluxUp + k, k);
    if (fluxDown) fluxDown[k] = normalised_column_flux(V, t, V.fluxDown + k, k);
    if (fluxAbsorbed) fluxAbsorbed[k] = normalised_column_flux(V, t, V.fluxAbsorbed + k, k);
  }
  if (volumeAbsorption)
    for (int kz = 0; kz < h->nz; ++kz)
      for (size_t k = 0; k < ncol; ++k) volumeAbsorption[(size_t)kz * ncol + k] = normalised_volume_absorption(V, t, kz, k);
  if (nDir > 0 && (intensity || intensityByComponent)) {
    // the column sums the excess of limited contributions is shared out by (:327-347), added up column after column
    std::vector<double> excessSums((size_t)(ncomp + 1) * nDir, 0.0);
    if (V.limitContrib)
      for (size_t jd = 0; jd < excessSums.size(); ++jd)
        for (size_t k = 0; k < ncol; ++k) excessSums[jd] += t[V.intensityByComponent + jd * ncol + k];
    for (int d = 0; d < nDir; ++d)
      for (size_t k = 0; k < ncol; ++k) {
        if (intensity) intensity[(size_t)d * ncol + k] = normalised_intensity(V, t, excessSums.data(), d, k);
        if (intensityByComponent)
          for (int j = 0; j <= ncomp; ++j)
            intensityByComponent[((size_t)j * nDir + d) * ncol + k] = normalised_intensity_by_component(V, t, excessSums.data(), j, d, k);
      }
  }
  return 0;
}

int i3rc_hip_normalise_level_fluxes(const i3rc_hip_integrator *h, const double *t, float *levelFluxUp, float *levelFluxDown) {
  if (!h || !t) return 1;
  if (h->extra != EXTRA_LEVELS) return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_normalise_level_fluxes: level fluxes are not switched on");
  const TallyView &V = h->view;
  const size_t ncol = (size_t)h->nx * h->ny;
  for (size_t e = 0; e < (size_t)(h->nz + 1) * ncol; ++e) {   // (level after level, as the block is laid out)
    if (levelFluxUp) levelFluxUp[e] = normalised_extra_value(V, t, EXTRA_LEVELS, V.levelUp, e);
    if (levelFluxDown) levelFluxDown[e] = normalised_extra_value(V, t, EXTRA_LEVELS, V.levelDown, e);
  }
  return 0;
}

int i3rc_hip_normalise_path_lengths(const i3rc_hip_integrator *h, const double *t, float *pathLengthUp, float *pathLengthSquaredUp, float *pathLengthDown,
                                    float *pathLengthSquaredDown) {
  if (!h || !t) return 1;
  if (h->extra != EXTRA_PATHS) return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_normalise_path_lengths: path lengths are not switched on");
  const TallyView &V = h->view;
  const size_t ncol = (size_t)h->nx * h->ny;
  float *const out[4] = {pathLengthUp, pathLengthSquaredUp, pathLengthDown, pathLengthSquaredDown};   // (as the block is laid out)
  for (int f = 0; f < 4; ++f)
    for (size_t k = 0; out[f] && k < ncol; ++k) out[f][k] = normalised_extra_value(V, t, EXTRA_PATHS, V.pathUp1, (long long)(f * ncol + k));
  return 0;
}

int i3rc_hip_normalise_radiance_path_lengths(const i3rc_hip_integrator *h, const double *t, float *radiancePathLength, float *radiancePathLengthSquared) {
  if (!h || !t) return 1;
  if (h->extra != EXTRA_RADIANCE_PATHS)
    return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_normalise_radiance_path_lengths: radiance path lengths are not switched on");
  const TallyView &V = h->view;
  const size_t n = (size_t)h->nDir * h->nx * h->ny;
  float *const out[2] = {radiancePathLength, radiancePathLengthSquared};   // (as the block is laid out)
  for (int f = 0; f < 2; ++f)
    for (size_t e = 0; out[f] && e < n; ++e) out[f][e] = normalised_extra_value(V, t, EXTRA_RADIANCE_PATHS, V.radiancePath1, (long long)(f * n + e));
  return 0;
}

int i3rc_hip_normalise_path_histogram(const i3rc_hip_integrator *h, const double *t, float *up, float *pathUp, float *down, float *pathDown) {
  if (!h || !t) return 1;
  if (h->extra != EXTRA_PATH_BINS) return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_normalise_path_histogram: the path histogram is not switched on");
  const long long block = extra_block_offset(h->layout.counters);
  float *const out[4] = {up, pathUp, down, pathDown};   // (as the block is laid out)
  for (int f = 0; f < 4; ++f)
    for (int b = 0; out[f] && b <= h->pathBins; ++b)
      out[f][b] = normalised_extra_value(h->view, t, EXTRA_PATH_BINS, block, path_bin_field(f, h->pathBins) + b);
  return 0;
}

int i3rc_hip_normalise_actinic_flux(const i3rc_hip_integrator *h, const double *t, float *actinicFlux) {
  if (!h || !t || !actinicFlux) return 1;
  if (h->extra != EXTRA_TRACKS) return const_cast<i3rc_hip_integrator *>(h)->fail("i3rc_hip_normalise_actinic_flux: the actinic flux is not switched on");
  const TallyView &V = h->view;
  const size_t ncol = (size_t)h->nx * h->ny;
  for (size_t e = 0; e < (size_t)h->nz * ncol; ++e) actinicFlux[e] = normalised_extra_value(V, t, EXTRA_TRACKS, track_block(h), e);
  return 0;
}

}  // extern "C"

namespace {
// The launch of the general flux kernel under the tag of the handle's extra tally block, through the one path every plain launch
// takes (defined last, so that these kernels are instantiated behind every other kernel of the library: the level kernels, then the
// track kernels, then the path kernels, then the histogram kernels, then the radiance path kernels).
int launch_extra(i3rc_hip_integrator *h, const Launch &L, const RunArgs &A, hipStream_t stream, bool timeIt) {
  switch (h->extra) {
    case EXTRA_LEVELS: return launch<PhiloxLevelStream>(h, L, A, stream, timeIt);
    case EXTRA_TRACKS: return launch<PhiloxTrackStream>(h, L, A, stream, timeIt);
    case EXTRA_PATHS: return launch<PhiloxPathStream>(h, L, A, stream, timeIt);
    case EXTRA_PATH_BINS: return launch<PhiloxBinStream>(h, L, A, stream, timeIt);
    case EXTRA_RADIANCE_PATHS: return launch<PhiloxRadiancePathStream>(h, L, A, stream, timeIt);
    case EXTRA_NONE: break;
  }
  return h->fail("internal: no extra tally block is switched on");
}

// The production instantiation of a stream's kernels for a key, null where there is none.  (A template only for when it is instantiated:
// behind the launches above.  The kernels of the code object stand in the order in which the launches first name their lists; a plain
// function that names the lists would be seen first and put them in its own order.)
template <int = 0>
const KernelEntry *find_kernel(const StreamKind &s, const KernelKey &key) {
  const std::vector<KernelEntry> &list = s.replay ? stream_kernels<ReplayStream>() : s.batched ? stream_kernels<PhiloxBatchStream>()
                                         : s.extra == EXTRA_LEVELS ? stream_kernels<PhiloxLevelStream>()
                                         : s.extra == EXTRA_TRACKS ? stream_kernels<PhiloxTrackStream>()
                                         : s.extra == EXTRA_PATHS ? stream_kernels<PhiloxPathStream>()
                                         : s.extra == EXTRA_PATH_BINS ? stream_kernels<PhiloxBinStream>()
                                         : s.extra == EXTRA_RADIANCE_PATHS ? stream_kernels<PhiloxRadiancePathStream>() : stream_kernels<PhiloxStream>();
  for (const KernelEntry &e : list)
    if (e.key == key) return &e;
  return nullptr;
}
EnvKnobs env_from_words(const int32_t *w) {
  if (!w) return EnvKnobs::process();
  EnvKnobs e;
  e.columns = w[0] != 0; e.ldsTallies = w[1] != 0; e.tableLds = w[2] != 0; e.plainPlaces = w[3]; e.fusedPlaces = w[4]; e.direct = w[5] != 0; e.cellRecords = w[6] != 0;
  return e;
}
}  // namespace

extern "C" {

/* Host only: the facts of a domain's field (launch_plan.hpp, derive_facts) as words -- binding.FACT_NAMES. */
int i3rc_hip_problem_facts(int nx, int ny, int nz, int ncomp, const float *xEdges, const float *yEdges, const float *zEdges, const float *totalExt,
                           const float *cumExt, const float *ssa, const int32_t *pfIndex, const int32_t *env, int32_t *out, int nout) {
  if (nx < 1 || ny < 1 || nz < 1 || ncomp < 1 || !xEdges || !yEdges || !zEdges || !totalExt || !cumExt || !ssa || !pfIndex || !out) return 2;
  ProblemFacts f;
  g_createError = derive_facts(f, env_from_words(env), nx, ny, nz, ncomp, xEdges, yEdges, zEdges, totalExt, cumExt, ssa, pfIndex);
  if (!g_createError.empty()) return 1;
  const int32_t v[kFactWords] = {f.nx, f.ny, f.nz, f.ncomp, f.xyRegular, f.zRegular, f.empty, f.absorbing, f.uniformSsa >= 0.f, f.uniformPf, f.cellRecBytes,
                                 f.colRecords, f.colBase, f.bsx, f.bsy, f.bsz, f.nbx, f.nby, f.nbz, f.clearShift, f.clearNx, f.clearWords,
                                 *std::max_element(f.maxPfIndex.begin(), f.maxPfIndex.end())};
  for (int k = 0; k < std::min(nout, kFactWords); ++k) out[k] = v[k];
  return 0;
}

/* Host only: what a launch of `kind` would be on a problem of these facts (i3rc_hip_problem_facts), this setup -- binding.SETUP_NAMES:
 * what the setters and the handle's knobs add -- and these switches of the process (binding.ENV_NAMES; NULL: the process's own).
 * kind: the stream (0 plain, 1 fused, 2 replay, 3 level tally, 4 track tally, 5 path tally, 6 path histogram, 7 radiance path tally), the kind of the source, the batches of a
 * fused launch and -- read for stream 6 only -- the histogram's bins. */
int i3rc_hip_plan_launch(const int32_t *facts, const int32_t *setup, const int32_t *env, const int32_t *kind, int32_t *out, int nout,
                         char *text, int ntext) {
  if (!facts || !setup || !kind || !out || !text || ntext < 1 || kind[0] < 0 || kind[0] > 7 || facts[3] < 1) return 2;
  if (kind[0] == 6 && (kind[3] < 1 || kind[3] > kMaxPathBins)) return 2;
  ProblemFacts f;
  f.nx = facts[0]; f.ny = facts[1]; f.nz = facts[2]; f.ncomp = facts[3]; f.xyRegular = facts[4]; f.zRegular = facts[5]; f.empty = facts[6] != 0;
  f.absorbing = facts[7] != 0; f.uniformSsa = facts[8] ? 0.5f : -1.f; f.uniformPf = facts[9]; f.cellRecBytes = facts[10];
  f.colRecords = facts[11] != 0; f.colBase = facts[12] != 0; f.bsx = facts[13]; f.bsy = facts[14]; f.bsz = facts[15]; f.nbx = facts[16];
  f.nby = facts[17]; f.nbz = facts[18]; f.clearShift = facts[19]; f.clearNx = facts[20]; f.clearWords = facts[21];
  f.maxPfIndex.assign(f.ncomp, facts[22]);
  static const float present = 0.f;
  CompTables t{};
  f.nDir = setup[0];
  t.inv = t.invCos = setup[1] ? &present : nullptr; t.fwd = t.fwdOrig = setup[2] ? &present : nullptr; t.nInv = setup[3];
  f.comp.assign(f.ncomp, t); f.nInvEntries.assign(f.ncomp, setup[4]); f.nFwdEntries.assign(f.ncomp, 0);
  f.params.useSurfaceBDRF = setup[5]; f.params.useRayTracing = setup[6]; f.nxs = setup[7]; f.nys = setup[8]; f.surfaceSet = setup[9] != 0;
  f.extra = (ExtraTally)setup[10]; f.kernelVariant = setup[11]; f.gridPlace = setup[12]; f.ldsTalliesOn = setup[13] != 0;
  f.pathBins = kind[0] == 6 ? kind[3] : 0;
  const StreamKind s = kind[0] == 2 ? stream_of<ReplayStream>() : kind[0] == 1 ? stream_of<PhiloxBatchStream>()
                                                                : plain_stream(kind[0] == 3 ? EXTRA_LEVELS : kind[0] == 4 ? EXTRA_TRACKS : kind[0] == 5 ? EXTRA_PATHS : kind[0] == 6 ? EXTRA_PATH_BINS : kind[0] == 7 ? EXTRA_RADIANCE_PATHS : EXTRA_NONE);
  const LaunchDecision d = plan_launch(f, env_from_words(env), {s, kind[1]});
  const KernelEntry *kern = d.refusal.empty() ? find_kernel(s, d.key) : nullptr;
  const std::string say = !d.refusal.empty() ? d.refusal : kern ? kern->name : no_kernel_text(s.batched);
  std::snprintf(text, (size_t)ntext, "%s", say.c_str());
  if (!kern) return 1;
  int32_t v[kPlanWords + 4];
  plan_words(f, d, kind[2], v);
  v[kPlanWords] = (int32_t)d.estimate; v[kPlanWords + 1] = d.rayQueueCap; v[kPlanWords + 2] = d.threads; v[kPlanWords + 3] = d.ldsBins;
  for (int k = 0; k < std::min(nout, kPlanWords + 4); ++k) out[k] = v[k];
  return 0;
}

}  // extern "C"

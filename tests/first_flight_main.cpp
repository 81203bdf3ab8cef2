// Host program over csrc/first_flight.hpp alone (tests/test_first_flight_cpu.py; build with -ffp-contract=off).
//   first_flight_main landing      holds first_flight_landing to a plain sequential restatement of the vertical trace -- one voxel step
//                                  after the other, `acc + step * ext > t`, the arrival's division -- on columns it makes itself, every
//                                  result compared with == (floats by their bits); prints one line of counts
//   first_flight_main elevated     the start layer of an elevated domain whose start height rounds to zMax, as the kernels find it
//   first_flight_main eligible     first_flight_eligible over a grid of all its inputs, one line per case
//   first_flight_main pack         flight_pack taken apart again by flight_ix / flight_iy / flight_code, one line per case
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "first_flight.hpp"

using namespace i3rc;

namespace {

uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
// Fortran's SPACING for real(4), as the kernels spell it (tracer.hpp, spacingf)
float spacingf(float x) {
  const uint32_t e = bits(x) & 0x7f800000u;
  return e > (23u << 23) ? from_bits(e - (23u << 23)) : FLT_MIN;
}

struct Column {
  int nz = 0;
  std::vector<float> zE;    // nz + 1 edges
  std::vector<float> ext;   // ext[iz], iz = 1 .. nz (ext[0] unused)
  float zStart = 0.f;
  int layer = 0;            // the start layer
};

// the Directional start height and its layer (photon_kernel: zStart, find_z on a regular grid -- on an irregular one the layer whose
// edges enclose the height, which is all the landing needs of it)
void set_start(Column &c, bool regular) {
  const float z0 = c.zE.front(), zMax = c.zE.back();
  c.zStart = z0 + (1.0f - spacingf(1.0f)) * (zMax - z0);
  if (regular) {
    const float deltaZ = c.zE[1] - c.zE[0];
    int k = (int)((c.zStart - z0) / deltaZ) + 1;
    k = k < c.nz ? k : c.nz;
    if (std::fabs(c.zE[k] - c.zStart) < spacingf(c.zStart)) k = k + 1;
    c.layer = k;
  } else {
    int k = c.nz;
    while (k > 1 && !(c.zE[k - 1] <= c.zStart)) --k;
    c.layer = c.zStart >= zMax ? c.nz + 1 : k;
  }
}

struct Walk { int steps, layer; float z; };
// The vertical trace as the tracer steps it (trace_step_lazy with dx = dy = 0, dz = -1, then finish_arrival): the step is the distance
// to the lower face divided by the cosine, the path grows by step * ext, the photon arrives where the grown path passes t -- and is
// then advanced by (t - path so far) / ext from where it stands --, else it stands on the face and is one layer further down.
// table (may be null): the path after every step that did not arrive.
Walk walk(const Column &c, float t, bool hasTarget, std::vector<float> *table) {
  const float dz = -1.0f;
  float acc = 0.0f, z = c.zStart;
  int iz = c.layer, steps = 0;
  if (table) table->assign(1, 0.0f);
  for (;;) {
    const float face = c.zE[iz - 1];
    const float step = (face - z) / dz;
    const float e = c.ext[iz];
    const float tauCell = step * e;
    ++steps;
    if (hasTarget && acc + tauCell > t) {
      const float rest = t - acc;
      const float part = rest / e;
      return {steps, iz, z + part * dz};
    }
    acc = acc + tauCell;
    if (table) table->push_back(acc);
    z = face;
    iz = iz - 1;
    if (iz < 1) return {steps, 0, 0.0f};
  }
}

struct Counts {
  long long cases = 0, mismatches = 0, columns = 0, bottom = 0, landed = 0, firstStep = 0, lastLayer = 0, onTable = 0, beyond = 0,
            clearAbove = 0, clearInside = 0, clearBelow = 0, allClear = 0, unequal = 0, tinyExt = 0, hugeExt = 0, notFinite = 0, lands = 0, notLands = 0;
};

void check(const Column &c, const std::vector<float> &A, float t, Counts &n) {
  if (!(t >= 0.0f)) return;   // (an optical depth is -log of a deviate in (0, 1])
  const Walk want = walk(c, t, true, nullptr);
  const FlightLanding got = first_flight_landing(
      [&](int k) { return A[k]; }, [&](int iz) { return c.ext[iz]; }, c.zE.data(), c.zStart, c.layer, -1.0f, t, [](float rest, float e) { return rest / e; });
  ++n.cases;
  const bool same = got.steps == want.steps && got.layer == want.layer && (want.layer == 0 || bits(got.z) == bits(want.z));
  if (!same) {
    if (n.mismatches < 5)
      std::fprintf(stderr, "mismatch: nz %d layer %d t %a: steps %d / %d layer %d / %d z %a / %a\n", c.nz, c.layer, t, got.steps, want.steps, got.layer,
                   want.layer, got.z, want.z);
    ++n.mismatches;
  }
  if (want.layer == 0) ++n.bottom; else ++n.landed;
  if (want.layer != 0 && want.steps == 1) ++n.firstStep;
  if (want.layer == 1) ++n.lastLayer;
  if (want.layer != 0) {
    const float surfaceZ = c.zE.front() + spacingf(c.zE.front());
    const bool finite = std::isfinite(want.z);
    if (!finite) ++n.notFinite;
    const bool lands = first_flight_lands(got.z, surfaceZ, c.zE.back());
    if (lands != (finite && want.z > surfaceZ && want.z < c.zE.back())) ++n.mismatches;
    if (lands) ++n.lands; else ++n.notLands;
  }
}

int landing() {
  std::mt19937 gen(20250117u);
  std::uniform_real_distribution<float> unit(0.0f, 1.0f);
  Counts n;
  for (int trial = 0; trial < 1500; ++trial) {
    Column c;
    c.nz = 1 + (int)(gen() % 64u);
    const bool regular = (trial & 1) == 0;
    const float z0 = (gen() % 7u == 0u) ? 0.5f : 0.0f;
    const float depth = std::ldexp(1.0f, (int)(gen() % 5u) - 3);   // 0.125 ... 2: equal depths add up exactly
    c.zE.assign(1, z0);
    for (int k = 1; k <= c.nz; ++k) c.zE.push_back(regular ? z0 + (float)k * depth : c.zE.back() + depth * (0.25f + unit(gen)));
    set_start(c, regular);
    if (c.layer < 1 || c.layer > c.nz) { --trial; continue; }   // (z0 = 0.5: some start heights round to zMax -- no launch lands from such a domain; another column)
    // extinctions: log-uniform over 1e-30 ... 1e4, and runs of clear layers above, inside and below the cloud
    c.ext.assign(c.nz + 1, 0.0f);
    const int kind = trial % 6;   // 0: cloud everywhere, 1: clear above, 2: clear below, 3: a clear gap inside, 4: all clear, 5: clear above and below
    const int a = 1 + (int)(gen() % (unsigned)c.nz), b = 1 + (int)(gen() % (unsigned)c.nz);
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int range = trial % 3;   // the whole span of exponents, thin, thick
    for (int iz = 1; iz <= c.nz; ++iz) {
      const float lg = range == 0 ? -30.0f + 34.0f * unit(gen) : (range == 1 ? -3.0f + 3.0f * unit(gen) : 4.0f * unit(gen));
      float e = std::pow(10.0f, lg);
      if (trial % 11 == 0 && iz == lo) e = 1e-30f;
      if (trial % 13 == 0 && iz == hi) e = 1e4f;
      bool clear = false;
      if (kind == 1) clear = iz > hi;
      if (kind == 2) clear = iz < lo;
      if (kind == 3) clear = iz >= lo && iz <= hi && c.nz >= 3 && lo > 1 && hi < c.nz;
      if (kind == 4) clear = true;
      if (kind == 5) clear = iz < lo || iz > hi;
      c.ext[iz] = clear ? 0.0f : e;
      if (!clear && e < 1e-20f) ++n.tinyExt;
      if (!clear && e >= 1e3f) ++n.hugeExt;
    }
    if (kind == 1 || kind == 5) ++n.clearAbove;
    if (kind == 2 || kind == 5) ++n.clearBelow;
    if (kind == 3) ++n.clearInside;
    if (kind == 4) ++n.allClear;
    std::vector<float> A;
    const Walk through = walk(c, 0.0f, false, &A);
    if (through.layer != 0 || (int)A.size() != c.layer + 1) { std::fprintf(stderr, "the table's sweep ended in layer %d\n", through.layer); return 2; }
    ++n.columns;
    if (!regular) ++n.unequal;
    // depths on both sides of every A[k]: the sum itself, the floats next to it, points between two sums; beyond A[nz]; random ones
    for (int k = 0; k <= c.layer; ++k) {
      const float s = A[k];
      check(c, A, s, n); ++n.onTable;
      check(c, A, std::nextafter(s, INFINITY), n);
      check(c, A, std::nextafter(s, -INFINITY), n);
      if (k > 0) { check(c, A, 0.5f * (A[k - 1] + s), n); check(c, A, A[k - 1] + unit(gen) * (s - A[k - 1]), n); }
    }
    const float total = A.back();
    for (float t : {total + 1.0f, 2.0f * total + 1e-30f, 87.5f > total ? 87.5f : total * 3.0f, FLT_MAX}) { check(c, A, t, n); if (t > total) ++n.beyond; }
    for (int i = 0; i < 40; ++i) check(c, A, -std::log(std::fmax(FLT_MIN, unit(gen))), n);
    check(c, A, 0.0f, n);
    check(c, A, FLT_MIN, n);
  }
  std::printf("cases %lld mismatches %lld columns %lld bottom %lld landed %lld firstStep %lld lastLayer %lld onTable %lld beyond %lld clearAbove %lld "
              "clearInside %lld clearBelow %lld allClear %lld unequal %lld tinyExt %lld hugeExt %lld notFinite %lld lands %lld notLands %lld\n",
              n.cases, n.mismatches, n.columns, n.bottom, n.landed, n.firstStep, n.lastLayer, n.onTable, n.beyond, n.clearAbove, n.clearInside,
              n.clearBelow, n.allClear, n.unequal, n.tinyExt, n.hugeExt, n.notFinite, n.lands, n.notLands);
  return n.mismatches == 0 ? 0 : 1;
}

// z0 = 4096, seven layers of 1 / 7 ... : the start height z0 + (1 - spacing(1)) (zMax - z0) rounds to zMax, find_z answers nz + 1
int elevated() {
  Column c;
  c.nz = 8;
  for (int k = 0; k <= c.nz; ++k) c.zE.push_back(4096.0f + 0.125f * (float)k);
  c.ext.assign(c.nz + 1, 1.0f);
  set_start(c, true);
  const bool ok = first_flight_eligible(true, 0, 0.0f, -0.0f, -1.0f, c.layer, 3, 5, c.nz, true);
  std::printf("zStart %a zMax %a layer %d nz %d eligible %d\n", c.zStart, c.zE.back(), c.layer, c.nz, ok ? 1 : 0);
  return 0;
}

int eligible() {
  const float zeros[5] = {0.0f, -0.0f, 1e-30f, -1e-7f, NAN};
  const float downs[3] = {-1.0f, -0.5f, 1.0f};
  const int sizes[3] = {1, 2047, 2048}, layers[3] = {1, 1022, 1023};
  for (int store = 0; store < 2; ++store)
    for (int src = 0; src < 2; ++src)
      for (float dx : zeros)
        for (float dy : zeros)
          for (float dz : downs)
            for (int nx : sizes)
              for (int ny : sizes)
                for (int nz : layers)
                  for (int start : {0, 1, nz, nz + 1})
                    for (int table = 0; table < 2; ++table)
                      std::printf("%d %d %08x %08x %08x %d %d %d %d %d %d\n", store, src, bits(dx), bits(dy), bits(dz), start, nx, ny, nz, table,
                                  first_flight_eligible(store != 0, src, dx, dy, dz, start, nx, ny, nz, table != 0) ? 1 : 0);
  return 0;
}

int pack() {
  for (int ix : {1, 2, 1024, kFlightMaxColumns})
    for (int iy : {1, 2, 1024, kFlightMaxColumns})
      for (int code : {kFlightBottom, 1, 512, kFlightMaxLayers, kFlightNotLanded}) {
        const int w = flight_pack(ix, iy, code);
        std::printf("%d %d %d %08x %d %d %d\n", ix, iy, code, (unsigned)w, flight_ix(w), flight_iy(w), flight_code(w));
      }
  std::printf("limits %d %d %d %d %u\n", kFlightMaxColumns, kFlightMaxLayers, kFlightBottom, kFlightNotLanded, kFirstFlight);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const char *what = argc > 1 ? argv[1] : "";
  if (!std::strcmp(what, "landing")) return landing();
  if (!std::strcmp(what, "elevated")) return elevated();
  if (!std::strcmp(what, "eligible")) return eligible();
  if (!std::strcmp(what, "pack")) return pack();
  std::fprintf(stderr, "usage: first_flight_main landing | elevated | eligible | pack\n");
  return 2;
}

// THE FIRST FLIGHT OF A ZENITH SUN, from a table per column (photon_kernel, STORE, part B -- "the fill"; kernels.hpp).
// With the sun at the zenith a Directional photon goes straight down its start column until its first event: dx = dy = +-0, dz = -1,
// so x and y never move (x + adv * 0), every step ends on a layer face, and the optical path after k steps is the SAME float32 sum for
// every photon of the column.  The specialised flux kernels of plain launches re-derived that sum step by step for every photon; here
// it is a table A[column][k], k = 0 .. nz, made once per integrator by the tracer's own step (first_flight_table_kernel), and the fill
// -- which makes 64 photons' starts at once, in uniform control flow -- looks the photon's first optical depth up in it and leaves
// the photon where its first scattering happens, or below the grid.
// Two pure functions and the slot's packing, host C++17 and device code alike, no HIP call: tests/first_flight_main.cpp holds the landing
// to a sequential restatement of the vertical trace (trace_step_lazy's `reach` test followed by finish_arrival), compared with ==.
#pragma once

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define I3RC_FLIGHT_FN __host__ __device__ __forceinline__
#else
#define I3RC_FLIGHT_FN inline
#endif

namespace i3rc {

// The launch lands its photons in the fill: one more bit of DevProblem::eventFlags (beside EventFlag's, event_flags.hpp), OR-ed in by
// the host where first_flight_eligible says so.  Wave-uniform: a launch's slots are all of one packing.
constexpr unsigned kFirstFlight = 16u;

// The slot's index word of such a launch: ix | iy << 11 | code << 22 -- code the landing layer (1 .. nz), 0 for a photon that crosses the
// whole column and leaves through the bottom, 1023 for one that is not landed and flies as before.  Hence the limits below.
constexpr int kFlightIyShift = 11, kFlightCodeShift = 22;
constexpr int kFlightMaxColumns = 2047, kFlightMaxLayers = 1022;   // nx, ny | nz
constexpr int kFlightBottom = 0, kFlightNotLanded = 1023;
I3RC_FLIGHT_FN int flight_pack(int ix, int iy, int code) { return ix | (iy << kFlightIyShift) | (code << kFlightCodeShift); }
I3RC_FLIGHT_FN int flight_ix(int word) { return word & ((1 << kFlightIyShift) - 1); }
I3RC_FLIGHT_FN int flight_iy(int word) { return (word >> kFlightIyShift) & ((1 << kFlightIyShift) - 1); }
I3RC_FLIGHT_FN int flight_code(int word) { return (int)((uint32_t)word >> kFlightCodeShift); }

// Is a launch eligible?
//   storeLaunch   a plain launch of a STORE kernel (has_start_store);  srcKind: i3rc_source::kind, 0 = Directional
//   solarDx/Dy/Dz the sun's direction cosines as upload_source makes them: the sun is at the zenith where dx and dy are zero, of either
//                 sign (0 * sin(phi) can be -0); a unit vector's dz is then -1 (upload_source: solarDz = -|mu|) -- held to that, since
//                 the landing's faces are those of a photon that goes DOWN
//   startLayer    find_z of the start height (the kernels' izStart): inside the grid, 1 .. nz -- a thin elevated domain's start height
//                 can round to zMax and its layer to nz + 1
//   tableExists   the column table has been made, and its sweep met no step <= 0, no NaN and no sum that fell
I3RC_FLIGHT_FN bool first_flight_eligible(bool storeLaunch, int srcKind, float solarDx, float solarDy, float solarDz, int startLayer, int nx, int ny, int nz,
                                          bool tableExists) {
  return storeLaunch && srcKind == 0 && solarDx == 0.0f && solarDy == 0.0f && solarDz == -1.0f && startLayer >= 1 && startLayer <= nz &&
         nx <= kFlightMaxColumns && ny <= kFlightMaxColumns && nz <= kFlightMaxLayers && tableExists;
}

// Where the vertical flight of one photon ends.
struct FlightLanding {
  int steps;   // voxel steps the tracer would have counted, the arriving one included
  int layer;   // the layer the photon stands in (the tracer's 1-based iz); 0: it left through the bottom after `startLayer` steps
  float z;     // its height (not set for layer 0: finish_exit puts such a photon at z0)
};
// A(k), k = 0 .. startLayer: the column's optical path after k downward steps from the start height (A[0] = 0; non-decreasing);
// ext(iz): the extinction of the column's cell in layer iz;  zE[k]: the layer edges;  zStart, startLayer: the start height and its layer;
// dz: the direction cosine (-1);  t: the photon's first optical depth;  divide(rest, ext): the quotient as finish_arrival forms it --
// exact_div by the refined reciprocal with its guard for ext < 1e-20 on the device, which is the IEEE quotient, `/` on the host.
// The tracer arrives in its k-th step where acc + step * ext > t with acc = A[k - 1], and acc + step * ext rounds to A[k] (no contraction:
// -ffp-contract=off): k is the smallest k with A[k] > t, found by bisection.  It then stands on the face it reached last -- the start
// height for k = 1, else the upper edge of its layer -- and finish_arrival advances it by (t - A[k - 1]) / ext.
template <class Table, class Ext, class Edges, class Divide>
I3RC_FLIGHT_FN FlightLanding first_flight_landing(const Table &A, const Ext &ext, const Edges &zE, float zStart, int startLayer, float dz, float t,
                                                  const Divide &divide) {
  int lo = 1, hi = startLayer + 1;   // the answer lies in [lo, hi]; startLayer + 1: no such k
  while (lo < hi) {
    const int mid = (int)((unsigned)(lo + hi) >> 1);
    if (A(mid) > t) hi = mid; else lo = mid + 1;
  }
  FlightLanding o;
  o.steps = lo > startLayer ? startLayer : lo;
  o.layer = lo > startLayer ? 0 : startLayer - lo + 1;
  o.z = 0.0f;
  if (o.layer != 0) {
    const float rest = t - A(lo - 1);
    const float part = divide(rest, ext(o.layer));
    const float face = lo == 1 ? zStart : zE[o.layer];
    o.z = face + part * dz;
  }
  return o;
}

// Is a landed height one the event phase takes for a scattering -- finite, strictly above the surface's height and below the top?
// (`r.z >= zMax` is an exit through the top there and `r.z <= surfaceZ` an arrival at the surface: such a photon flies as before.)
I3RC_FLIGHT_FN bool first_flight_lands(float z, float surfaceZ, float zMax) {
  union { float f; uint32_t u; } b;
  b.f = z;
  return (b.u & 0x7f800000u) != 0x7f800000u && z > surfaceZ && z < zMax;
}

}  // namespace i3rc

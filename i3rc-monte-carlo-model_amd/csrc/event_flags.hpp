// What the event phase of the specialised flux kernels of plain launches (photon_kernel, STORE; kernels.hpp) would otherwise work out
// per lane, or by a float compare on scalar operands (gfx950 has no scalar float compare: they come out as v_cmp_*_f32_e64), although
// the launch decides it: ONE word of facts, DevProblem::eventFlags, made on the host by a pure function and tested on the device with
// scalar integer instructions.  Host C++17 and device code alike, no HIP call: tests/test_event_flags_cpu.py holds event_flags to the
// kernels' own expressions, restated there.
#pragma once

#include <cfloat>

namespace i3rc {

enum EventFlag : unsigned {
  // No photon's weight ever leaves 1: nothing absorbs (below), and a reflection either cannot happen or ends the photon -- a uniform
  // Lambertian surface whose albedo is at most tiny (`w * albedo <= tiny` with w = 1).  Then `w < 0.5` never holds and the roulette
  // is never played, whatever useRussianRoulette says.
  kWeightStaysOne = 1u,
  // Every cell shares one single-scattering albedo and it is at least 1: `ssa < 1` is false for every scattering of the launch.
  kNoAbsorption = 2u,
  // A scattering needs the index of its cell: the kernels' `needCell` of a one-component domain -- the cells do not share their
  // single-scattering albedo, or share one below 1 (the absorption is tallied per cell), or do not share their table entry.
  kNeedCell = 4u,
  // The launch can play Russian roulette: the caller asks for it, and some photon's weight can fall below 1 (kWeightStaysOne is clear).
  kPlaysRoulette = 8u,
};

// uniformSsa: >= 0 the value every cell shares, < 0 (or NaN) per-cell values; uniformPf: >= 1 the table entry every cell shares, else 0;
// brdfGrid: the surface's reflectance is looked up per reflection (DevProblem::useBDRF after a uniform grid has been folded into the
// albedo); albedo: the Lambertian albedo the kernels multiply by otherwise.
// useRoulette: the caller's useRussianRoulette (DevProblem::useRR); the callers from before the bit existed leave it out.
inline unsigned event_flags(float uniformSsa, int uniformPf, bool brdfGrid, float albedo, bool useRoulette = false) {
  unsigned f = 0u;
  const bool noAbsorption = uniformSsa >= 1.0f;
  if (noAbsorption) f |= kNoAbsorption;
  if (noAbsorption && !brdfGrid && albedo <= FLT_MIN) f |= kWeightStaysOne;
  if (!(uniformSsa >= 0.0f) || uniformSsa < 1.0f || uniformPf < 1) f |= kNeedCell;
  if (useRoulette && (f & kWeightStaysOne) == 0u) f |= kPlaysRoulette;
  return f;
}

}  // namespace i3rc

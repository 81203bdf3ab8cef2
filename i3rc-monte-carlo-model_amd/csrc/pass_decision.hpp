// What a wave of the specialised flux kernels of plain launches (photon_kernel, STORE; kernels.hpp) does in one pass of its loop,
// decided from the head's three lane counts as ONE small integer:
//   stop       nothing is left: no lane waits for an event, none turns over, none traces -- the loop ends;
//   runEvent   the pass runs its event phase: evThr lanes have an interaction due, or kTurnForce lanes wait to turn over, or no lane
//              is left to trace (and some lane waits);
//   doTurn     an event phase serves the turnover lanes too: kTurnMin of them have gathered, or no lane traces, or no lane scatters.
// The three are what the loop spelt as booleans,
//   stop     = nSc == 0 && nTu == 0 && trEmpty
//   runEvent = nSc + nTu > 0 && (nSc >= evThr || nTu >= kTurnForce || trEmpty)
//   doTurn   = nTu >= kTurnMin || trEmpty || nSc == 0,
// which the compiler keeps as 64-bit lane masks: every wave-uniform compare an s_cmp + s_cselect_b64 -1 / 0, joined by s_or_b64 /
// s_and_b64 and copied to vcc to be branched on.  Here they are 32-bit integer arithmetic that stays in SCC and 32-bit scalar registers:
// `a >= b` of two counts is the sign of b - 1 - a, an OR of conditions the sign of the differences' OR, and a wave with nothing to
// trace -- rare: a launch's last passes -- is one select.  `nSc + nTu > 0` needs no instruction: with evThr >= 1 and kTurnForce >= 1 the
// first two arms of runEvent imply it, and in the third it fails only where the wave stops.
// Where the wave stops the other two bits are set as well (kPassStop | kPassEvent | kPassTurn; the boolean runEvent was false there): the
// loop tests kPassStop first and leaves, so nobody reads them -- clearing the event bit would cost an instruction at every pass.
// Requires 0 <= nSc, nTu <= 64 and 1 <= evThr (i3rc_hip_set_tuning takes 1 ... 64, the adaptive rule gives 12 ... 44).
// Host C++17 and device code alike, no HIP call: tests/test_pass_decision_cpu.py holds the function to the three expressions above.
#pragma once

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define I3RC_PASS_FN __host__ __device__ __forceinline__
#else
#define I3RC_PASS_FN inline
#endif

namespace i3rc {

enum PassBits : int { kPassStop = 1, kPassEvent = 2, kPassTurn = 4 };

// 1 where x < 0, else 0
I3RC_PASS_FN int pass_sign(int x) { return (int)((uint32_t)x >> 31); }

// nSc, nTu: lanes with an interaction due / waiting to turn over; trEmpty: no lane traces
template <int kTurnMin, int kTurnForce>
I3RC_PASS_FN int pass_decision(int nSc, int nTu, bool trEmpty, int evThr) {
  static_assert(kTurnMin >= 1 && kTurnForce >= 1, "a quorum of no lanes would run event phases for nobody");
  static_assert(kTurnMin <= 64 && kTurnForce <= 64, "a wavefront has 64 lanes");
  // (nothing to trace: whoever waits is served now, the turnover lanes included -- one select on an INPUT of the arithmetic below: a full
  // wavefront of turnover lanes meets both quorums.  No branch: behind one, the two arms' bits were put together in a register and
  // taken apart again at every pass, whichever way it was written)
  const int turners = trEmpty ? 64 : nTu;
  const int event = pass_sign((evThr - 1 - nSc) | (kTurnForce - 1 - turners));   // nSc >= evThr || nTu >= kTurnForce || trEmpty
  const int turn = pass_sign((kTurnMin - 1 - turners) | (nSc - 1));              // nTu >= kTurnMin || trEmpty || nSc == 0
  // stop: trEmpty and nobody waits.  turners - 2 nTu - nSc is 64 there and nowhere else: 64 less something positive where trEmpty and
  // somebody waits, -nTu - nSc <= 0 where a lane traces
  const int stop = turners - (2 * nTu + nSc) == 64 ? 1 : 0;
  return stop * kPassStop + event * kPassEvent + turn * kPassTurn;
}

}  // namespace i3rc

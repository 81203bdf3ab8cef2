// Compile-time tuning knobs of photon_kernel (kernels.hpp): every default in one place, each with the measurement that chose it.
// A side build overrides a knob on the compiler's command line (-DI3RC_...=value: tools/variant_bench.py, tools/phase_profile.py,
// tools/locality_experiment.py).  Knobs without a value (-DI3RC_NESTED_BUILD, -DI3RC_PROFILE_PHASES, -DI3RC_FAST_ACOS, ...) are
// tested with #ifdef where they act.
#pragma once

// ---- waves per SIMD the compiler plans each kind of instantiation for (planned_waves, kernels.hpp)
#ifndef I3RC_RADIANCE_WAVES
#define I3RC_RADIANCE_WAVES 5   /* (the Landsat + 7 directions case gains 9 % over 4; 6 would spill) */
#endif
#ifndef I3RC_MIN_WAVES
#define I3RC_MIN_WAVES 5
#endif
// The specialised flux kernels need 54 vector registers: told to plan for eight waves per SIMD (instead of five) the
// compiler schedules them differently -- step cloud 3.13 -> 3.27e9 photons/s on the same box, 32 layers 2.56 -> 2.67e9,
// radar 640 flux 1.24 -> 1.29e9, Landsat-36 -0.5 %; the bricked kernels (at most five workgroups per CU anyway) lose 1 %.
#ifndef I3RC_FLUX_WAVES
#define I3RC_FLUX_WAVES 8
#endif
// (the fused multi-batch kernels carry five more vector registers per lane -- the batch and the per-lane counts -- and want 66:
// planned for seven waves per SIMD they keep them all; for eight, two go to scratch and nothing is gained: 2.97 against
// 2.83 ... 3.06e9 photons/s on the step cloud, 1.22 against 1.08e9 on the radar field, within the noise elsewhere)
#ifndef I3RC_FUSED_WAVES
#define I3RC_FUSED_WAVES 7
#endif
// (the radiance kernels for several components carry the stream's cursor and the component on top of the one-component kernels' 96
// registers: planned for five waves per SIMD they keep 4 ... 14 of them in scratch; measured against four waves: DESIGN.md section 8)
#ifndef I3RC_MULTI_WAVES
#define I3RC_MULTI_WAVES 4
#endif

// ---- absorption: a photon's consecutive scatterings in one cell leave as one atomic (photon_kernel, MERGE)
#ifndef I3RC_MERGE_ABSORPTION
#define I3RC_MERGE_ABSORPTION 1
#endif
// ---- a scattering reads what it needs of its cell as one record where the domain has such records (photon_kernel, part C)
#ifndef I3RC_CELL_RECORD_READS
#define I3RC_CELL_RECORD_READS 1
#endif

// ---- the schedule of ray mode and of the photons' event phase
#ifndef I3RC_STEP_AHEAD
#define I3RC_STEP_AHEAD 2
#endif
#ifndef I3RC_LOW_WATER
#define I3RC_LOW_WATER 64   /* = the ready buffer: with nothing left to expand, a wave leaves its rays unless a whole wavefront of them is in hand */
#endif
#ifndef I3RC_THIRD_STEP
#define I3RC_THIRD_STEP 4   /* a third ray step per pass when the service phase is this much further away: Landsat + 7 directions +2.4 % */
#endif
#ifndef I3RC_TURN_MIN
#define I3RC_TURN_MIN 4
#endif
#ifndef I3RC_TURN_FORCE
#define I3RC_TURN_FORCE 12
#endif
// ... of the flux kernels that start their photons from a start store (photon_kernel, STORE): a turnover lane there reads four words
// instead of working out its photon's start, so the quorum that kept that arithmetic from running at two or three lanes has less to
// protect.  Measured (step cloud, 1e8 photons, ms per step, two runs each | Landsat-36): quorum 1 27.49 / 27.47 | 75.3 / 75.8; 2 27.17 / 27.17 |
// 74.2 / 75.8; 2 with forced turnover 8 27.22 / 27.22 | 74.3 / 74.5; 1 with 6 27.43 / 27.44 | 76.1 / 77.6; 4 with 12 26.98 ... 27.05 | 74.0 / 74.4: the
// other kernels' values stay the best -- the quorum saves the CLOSING of a photon at two or three lanes as well (profiles/r07_start_store.txt)
#ifndef I3RC_STORE_TURN_MIN
#define I3RC_STORE_TURN_MIN 4
#endif
#ifndef I3RC_STORE_TURN_FORCE
#define I3RC_STORE_TURN_FORCE 12
#endif
// round 14, the same six kernels: wave-uniform and single-lane work taken out of their phases, one switch per item so that each can be
// measured against the tree without it (profiles/r14_uniform_work.txt; 0 = the kernels of round 13)
#ifndef I3RC_WRAP_PER_AXIS
#define I3RC_WRAP_PER_AXIS 1   /* the periodic wrap of the photon step: x behind its own mask, y behind its own */
#endif
#ifndef I3RC_EVENT_FLAGS
#define I3RC_EVENT_FLAGS 1     /* DevProblem::eventFlags decides absorption, the cell index and the roulette block for the launch */
#endif
#ifndef I3RC_TABLE_RCP_ONCE
#define I3RC_TABLE_RCP_ONCE 1  /* the inverse table's reciprocal length once per wave, not once per scattering */
#endif
// round 15, the same six kernels: how their photon step spells addresses and its outcome -- the float operations and their order are
// untouched; one switch per item, 0 = the kernels of round 14 (profiles/r15_step_addressing.txt)
#ifndef I3RC_STEP_BIASED_ADDRESS
#define I3RC_STEP_BIASED_ADDRESS 1   /* the extinction read's address (and the event phase's one cell index) in the biased-base form of cell_address.hpp */
#endif
#ifndef I3RC_STEP_STATE_SELECTS
#define I3RC_STEP_STATE_SELECTS 1    /* the lane state after a step: one chain of selects on the step's own masks, the bottom's value a scalar */
#endif
#ifndef I3RC_STEP_COLD_ERROR
#define I3RC_STEP_COLD_ERROR 1       /* the error exit of the step (no workload takes it) behind one uniform branch, its defaults inside */
#endif
// round 16, the same six kernels: the scalar work of the loop's head and of the event phase's masks -- only how a pass is decided is
// spelt anew, not what is decided; one switch per item, 0 = the kernels of round 15 (profiles/r16_pass_logic.txt)
#ifndef I3RC_PASS_DECISION
#define I3RC_PASS_DECISION 1         /* stop, runEvent and doTurn as the bits of one 32-bit scalar: pass_decision.hpp */
#endif
#ifndef I3RC_TURN_STATE_RANGE
#define I3RC_TURN_STATE_RANGE 1      /* the lane states numbered so that the three turnover states end the range: `wantTurn` one compare */
#endif
#ifndef I3RC_TURN_ALL_WORD
#define I3RC_TURN_ALL_WORD 1         /* doTurn as a 64-bit -1 / 0 word made once per event phase: every `mask & turnAll` one s_and_b64 */
#endif
// round 17, the same six kernels: scalar work that re-derives per phase what the launch decides once, or turns lane masks around with
// scalar logic another spelling does not need -- no float operation changes; one switch per item, 0 = the kernels of round 16
// (profiles/r17_scalar_relief.txt)
#ifndef I3RC_ROULETTE_FLAG
#define I3RC_ROULETTE_FLAG 1         /* "this launch can play roulette" as the bit kPlaysRoulette of DevProblem::eventFlags, not useRR and a second bit */
#endif
#ifndef I3RC_STEP_ADVANCE_MASKS
#define I3RC_STEP_ADVANCE_MASKS 1    /* the step's face masks as `quotient <= advance` (0 on an arriving lane): no scalar AND with !reach */
#endif
// round 18, the same six kernels: the first flight of a zenith sun's photons -- straight down their start column -- from a table of the
// column's cumulative optical path, looked up where the wave makes its photons' starts (first_flight.hpp; photon_kernel, FLIGHT); 0 = the
// kernels of round 17.  One build runs a launch both ways: I3RC_FIRST_FLIGHT_TABLE=0 in the environment, or
// i3rc_hip_set_first_flight_table (profiles/r18_first_flight.txt)
#ifndef I3RC_FIRST_FLIGHT_TABLE
#define I3RC_FIRST_FLIGHT_TABLE 1
#endif
#ifndef I3RC_PHOTON_STEP_AHEAD
#define I3RC_PHOTON_STEP_AHEAD 64   /* off: measured -1.6 % (step cloud) ... +2.8 % (Landsat-36), -3 % on the radar field */
#endif
// measured (Landsat + 7 directions, 2e7 photons, before the lazy roulette): low water 16 / 32 / 48 / 56 / 64 -> 3.1 / 4.2 / 4.6 / 4.7 /
// 4.7e7 photons/s; two steps per pass +8 %.  With the lazy roulette (most rays end in EXPAND): low water 40 / 48 / 56 / 64 ->
// 8.2 / 9.1 / 9.2 / 9.4e7 (radar-64 + nadir 5.8 / 5.9 / 6.1 / 6.2e8); expand batch 16 / 32 / 48 / 64 -> radar-64 5.8 / 6.1 /
// 6.3 / 6.4e8; both at 64: +5.5 % (radar-64), +3 % (Landsat + 7 directions), +4 % (radar 640 + nadir)
#ifndef I3RC_EXPAND_BATCH
#define I3RC_EXPAND_BATCH 64   /* = the ready buffer: expand when it is empty, a whole wavefront at a time */
#endif
// DIRECT: rays are traced once this many survivors are ready (or when the next event phase's rays would not fit into the store
// of 128: wantSlots), and the wave goes back to its photons when nothing is left to hand out and fewer than
// kDirectLeave rays are still under way (those few go back to the store: with rays of one or two voxel steps, a wave that
// left with a wavefront's worth under way -- the ring mode's rule -- would write back and take up again most of its rays)
#ifndef I3RC_DIRECT_ENTER
#define I3RC_DIRECT_ENTER 96   /* (radar-64 + nadir, 5e7 photons: 64 -> 59.1 ms, 80 -> 58.8, 96 -> 58.2, 112 -> 58.3; leave level 8 ... 48: within 1 %) */
#endif
#ifndef I3RC_DIRECT_LEAVE
#define I3RC_DIRECT_LEAVE 24
#endif

// ---- the thresholds a wave fits to its own photons (photon_kernel, adapt_thresholds)
// (round 4, the step phase a third cheaper than it was: 44 - slope * steps per event fits the measured optima -- step cloud 36 ... 40
// at 2.5 steps per event, Landsat-36 28 at 9.5, Landsat-119 18 ... 20 at 15 -- where 58 / sqrt(steps per event) sat below them on
// the long traces; radiance kernels, whose photons share the wave's time with their rays, want the flatter slope)
#ifndef I3RC_EVTHR_SLOPE_FLUX
#define I3RC_EVTHR_SLOPE_FLUX 2.0f
#endif
#ifndef I3RC_EVTHR_SLOPE_RADIANCE
#define I3RC_EVTHR_SLOPE_RADIANCE 1.2f
#endif
#ifndef I3RC_LITHR_COEF
#define I3RC_LITHR_COEF 70.0f
#endif
#ifndef I3RC_LITHR_MIN
#define I3RC_LITHR_MIN 16
#endif

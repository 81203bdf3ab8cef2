// The byte address of a cell's word in a field of 4-byte words laid out [nz][ny][nx] behind `base`, from the cell's 1-based indices:
//   4 * cell_index(ix, iy, iz) + base,   cell_index = (iz - 1) nx ny + (iy - 1) nx + (ix - 1)   (tracer.hpp)
// with the three `- 1` and the base folded into ONE launch-uniform bias,
//   bias = base - 4 (nx ny + nx + 1),   address = ((iz nx ny + ix) + iy nx) << 2) + bias,
// which the vector unit forms with two 24-bit multiplies, a three-way add and a shift-and-add where the spelled-out form took nine
// instructions (the photon step of the specialised flux kernels of plain launches: trace_step_lazy, STEP_BIASED; cell_extinction_biased).
// Equal to 4 * cell_index + base, modulo 2^32, under the conditions i3rc_hip_create guarantees for every grid:
//   nx ny < 2^24 and every index < 2^24   (the 24-bit multiplies take their operands' low 24 bits and give the product's low 32),
//   nx ny nz < 2^30                       (so that 4 * cell_index itself is below 2^32);
// the arithmetic is unsigned and wraps: a base smaller than 4 (nx ny + nx + 1) -- base 0, a field at the front of LDS -- gives a bias
// that is NEGATIVE read as an int, and the sum comes out right all the same.  The intermediate iz nx ny + iy nx + ix exceeds the
// cell index by nx ny + nx + 1 and may pass 2^30; shifted left by two it wraps, as the bias did.
// Host C++17 and device code alike, no HIP call: tests/test_cell_address_cpu.py holds both functions to 4 * cell_index + base.
#pragma once

#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define I3RC_CELL_FN __host__ __device__ __forceinline__
#else
#define I3RC_CELL_FN inline
#endif

namespace i3rc {

// the low 32 bits of the product of the operands' low 24 bits (v_mul_u32_u24 / v_mad_u32_u24 on the device)
I3RC_CELL_FN uint32_t cell_mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, b);
#else
  return (a & 0xffffffu) * (b & 0xffffffu);
#endif
}

// base: the byte address of cell (1, 1, 1)'s word (an LDS address, or the low word of a global one)
I3RC_CELL_FN uint32_t cell_address_bias(uint32_t base, int nx, int ny) {
  return base - 4u * ((uint32_t)nx * (uint32_t)ny + (uint32_t)nx + 1u);
}

// ix, iy, iz: 1-based, inside the grid.  cell_word: cell_index + (nx ny + nx + 1), the word the bias counts from (below 2^31)
I3RC_CELL_FN uint32_t cell_word(int nx, int ny, int ix, int iy, int iz) {
  const uint32_t planes = cell_mul24((uint32_t)iz, (uint32_t)nx * (uint32_t)ny) + (uint32_t)ix;
  return planes + cell_mul24((uint32_t)iy, (uint32_t)nx);
}
I3RC_CELL_FN uint32_t cell_address(uint32_t bias, int nx, int ny, int ix, int iy, int iz) {
  return (cell_word(nx, ny, ix, iy, iz) << 2) + bias;
}

// the same for the columns of a [ny][nx] field of records of (1 << shift) bytes: (((iy - 1) nx + (ix - 1)) << shift) + base
I3RC_CELL_FN uint32_t column_address_bias(uint32_t base, int nx, int shift) { return base - (((uint32_t)nx + 1u) << shift); }
I3RC_CELL_FN uint32_t column_address(uint32_t bias, int nx, int ix, int iy, int shift) {
  return ((cell_mul24((uint32_t)iy, (uint32_t)nx) + (uint32_t)ix) << shift) + bias;
}

}  // namespace i3rc

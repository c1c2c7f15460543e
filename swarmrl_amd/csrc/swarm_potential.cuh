// Gridded external potential (EspressoMD.add_external_potential,
// espresso.py:995-1036): a periodic scalar field phi[nx][ny][nz] with value
// [i][j][k] at the cell centre ((i + .5) hx, (j + .5) hy, (k + .5) hz),
// interpolated (tri)linearly; the force on a particle is minus the gradient
// of the interpolant at its folded position (the uint32 box fraction q; image
// counters do not enter).
//
// One fixed fp32 sequence ("External potential"), plain
// multiplies, adds and subtracts (the library is built with
// -ffp-contract=off), restated operation for operation in numpy by
// tests/potential_ref.py.  Per axis a with n cells:
//   P  = (uint64) q * n                          (< n 2^32)
//   P' = (P + n 2^32 - 2^31) mod (n 2^32)        (half a cell down, periodic)
//   i0 = P' >> 32,  i1 = (i0 + 1) mod n
//   t  = (float)((uint32) P' >> 8) * 2^-24       (exact, in [0, 1))
// 2-D, p_xy = phi[i_x][i_y]:
//   a = p10 - p00, b = p11 - p01, gx = a + ty (b - a), Fx = -(gx inv_hx)
//   c = p01 - p00, d = p11 - p10, gy = c + tx (d - c), Fy = -(gy inv_hy)
// 3-D: for the gradient along an axis the four differences along it at the
// corners of the other two axes b < c, interpolated along b, then along c.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace swarm {

// The field of an engine (Derived::pot).  phi == nullptr: no field.
// 3-D engines: phi is the plain array [n0][n1][n2].  2-D engines (n2 = 1):
// phi holds one 16-byte record of the four corners per cell,
//   rec[i0x][i0y] = {p00, p10, p01, p11},  p_ab = phi[(i0x + a) mod n0][(i0y + b) mod n1],
// built by the host (swarm_engine_set_potential_field): one load per lookup
// and no i1 arithmetic, at four times the memory.
struct PotentialField {
  const float* phi;  // device
  int32_t n[3];
  float inv_h[3];  // (float)(1 / h_a), h_a in fp64
};

// Grid cell and weight of box fraction q along an axis of n cells.
struct PotAxis {
  uint32_t i0, i1;
  float t;
};

__device__ __forceinline__ PotAxis pot_axis(uint32_t q, uint32_t n) {
  const uint32_t hi = __umulhi(q, n), lo = q * n;
  const uint32_t lo2 = lo - 0x80000000u;
  const uint32_t h1 = hi - (lo < 0x80000000u ? 1u : 0u);  // the borrow
  PotAxis r;
  r.i0 = h1 > hi ? n - 1u : h1;  // wrapped below zero: the last cell
  r.i1 = r.i0 + 1u == n ? 0u : r.i0 + 1u;  // (3-D only: the 2-D records hold the wrap)
  r.t = (float)(lo2 >> 8) * 5.9604644775390625e-08f;
  return r;
}

// 2-D: the cell's four corner values (one 16-byte load of its record, issued
// here) and the weights; the force from them later (pot_force2), so a kernel
// can put work in between.
struct PotSample2 {
  float p00, p10, p01, p11, tx, ty;
};

__device__ __forceinline__ PotSample2 pot_fetch2(const float* __restrict__ rec, uint32_t nx,
                                                 uint32_t ny, uint32_t qx, uint32_t qy) {
  const PotAxis x = pot_axis(qx, nx), y = pot_axis(qy, ny);
  const float4 c = reinterpret_cast<const float4*>(rec)[x.i0 * ny + y.i0];
  PotSample2 s;
  s.p00 = c.x;
  s.p10 = c.y;
  s.p01 = c.z;
  s.p11 = c.w;
  s.tx = x.t;
  s.ty = y.t;
  return s;
}

__device__ __forceinline__ void pot_force2(const PotSample2& s, float inv_hx, float inv_hy,
                                           float* Fx, float* Fy) {
  const float a = s.p10 - s.p00, b = s.p11 - s.p01;
  const float gx = a + s.ty * (b - a);
  const float c = s.p01 - s.p00, d = s.p11 - s.p10;
  const float gy = c + s.tx * (d - c);
  *Fx = -(gx * inv_hx);
  *Fy = -(gy * inv_hy);
}

// The force of the field on a particle at box fractions (qx, qy, qz).
// DIMS = 2: the field has one cell along z; F[2] = 0.
template <int DIMS>
__device__ __forceinline__ void potential_force(const PotentialField& f, uint32_t qx, uint32_t qy,
                                                uint32_t qz, float* F) {
  if (DIMS == 2) {
    const PotSample2 s =
        pot_fetch2(f.phi, (uint32_t)f.n[0], (uint32_t)f.n[1], qx, qy);
    pot_force2(s, f.inv_h[0], f.inv_h[1], &F[0], &F[1]);
    F[2] = 0.0f;
    return;
  }
  const uint32_t ny = (uint32_t)f.n[1], nz = (uint32_t)f.n[2];
  const PotAxis x = pot_axis(qx, (uint32_t)f.n[0]), y = pot_axis(qy, ny), z = pot_axis(qz, nz);
  const uint32_t ix[2] = {x.i0, x.i1}, iy[2] = {y.i0, y.i1}, iz[2] = {z.i0, z.i1};
  float p[2][2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 2; ++k) p[i][j][k] = f.phi[(ix[i] * ny + iy[j]) * nz + iz[k]];
  float u[2];
  // x: differences along x at (y, z), along y, then along z
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float d0 = p[1][0][k] - p[0][0][k], d1 = p[1][1][k] - p[0][1][k];
    u[k] = d0 + y.t * (d1 - d0);
  }
  F[0] = -((u[0] + z.t * (u[1] - u[0])) * f.inv_h[0]);
  // y: differences along y at (x, z), along x, then along z
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float d0 = p[0][1][k] - p[0][0][k], d1 = p[1][1][k] - p[1][0][k];
    u[k] = d0 + x.t * (d1 - d0);
  }
  F[1] = -((u[0] + z.t * (u[1] - u[0])) * f.inv_h[1]);
  // z: differences along z at (x, y), along x, then along y
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float d0 = p[0][j][1] - p[0][j][0], d1 = p[1][j][1] - p[1][j][0];
    u[j] = d0 + x.t * (d1 - d0);
  }
  F[2] = -((u[0] + y.t * (u[1] - u[0])) * f.inv_h[2]);
}

}  // namespace swarm

// Pairwise identity by descent (driven from kgx_pair_hmm.hip: kgx_pair_hmm): for every unordered pair of genomes the forward pass
// of the two-state hidden Markov model of include/kgx.h along the listed rows, with the smoothed IBD weight carried beside it, over
// k_pair_counts' genome-major panel (kgx_kernels_panel.h).  The library's first floating-point pairwise kernel: fp64 on the vector
// ALU.  The matrix cores have nothing to take here -- the step is a 2 x 2 product whose matrix differs per pair AND per row.
//
// k_pair_hmm: a workgroup of 256 threads owns a pair (A <= B) of 32-genome tiles for the WHOLE list (k_pair_runs' ownership: one
//   launch per row batch, no row slicing, no atomics).  Thread t walks genome t & 31 of A against the four genomes 4 (t >> 5) .. + 3
//   of B: four states {F0, F1, V0, V1} and their shared binary exponent E stay in registers over the batch (40 VGPRs); the device
//   table carries them from batch to batch (40 bytes a pair), so batching changes nothing.
//   Per step the workgroup stages ONE 64-row tile in LDS, two buffers, the next tile's words in flight in registers while this one
//   is walked, one barrier a tile:
//     codes[dword][genome]     the tile's 16 bytes of each of its 64 genomes as the panel has them (dword u: rows 16 u .. + 15);
//     table[row][ca][cb]       {e0, e1} as two doubles for every ORDERED pair of codes: thread t expands row t >> 2, code ca = t & 3
//                              from the row's twelve floats (the class k of include/kgx.h; 1, 1 where either code is 3) -- so the
//                              cell rule, the float -> double conversion and the no-call are paid once a (row, workgroup), not
//                              once a pair.
//   In the walk a pair and row cost one v_bfe_u32, one v_lshl_add_u32 and ONE ds_read_b128 at table + 256 row + 64 ca + 16 cb (the
//   row is an immediate offset; a row's sixteen entries are the 64 banks once, equal entries broadcast: no conflict) and then the
//   recursion: 2 adds, 8 multiplies, 5 fused multiply-adds -- 15 fp64 issue slots, no division, no log, no branch.  An fma rounds
//   once where the written form rounds twice and every term stays non-negative, so include/kgx.h's error bound holds with room.
//   rho, c0, c1 and w of the row are uniform over the workgroup: they come by scalar loads (32 bytes a row, sixteen rows ahead) and
//   enter the arithmetic as SGPR operands -- no LDS strip, no select.  (The other way round -- the twelve floats by scalar loads and a
//   v_cndmask chain over the six classes -- costs 2 x 2 x 6 selects and two conversions a pair-row, more than the recursion.)
//   Every 16 list positions (fixed positions of the list: first_row is a multiple of 64) the four values are scaled by 2^-k, k the
//   exponent of F0 + F1, and E += k: exact, 7 slots a pair and 16 rows.
//   Nothing in the walk depends on the data: the rows past the list's end in its last 16-row group are identities (rho = 1, c = 0,
//   w = 0, e = 1: every product and fma exact), which the driver's padding supplies; a lane whose pair is not in the table (a > b on
//   a diagonal tile pair, a genome past the last, a masked genome) computes on whatever the panel holds and stores nothing of it.
//   The last batch turns the state into {ln(F0 + F1) + E ln 2, (V0 + V1) / (F0 + F1)}: one log and one division a pair.
#pragma once

#include <cstdint>

#include "kgx_kernels_common.h"

namespace kgx {

constexpr uint32_t kHmmTile = 32;                                             // genomes of a tile side
constexpr uint32_t kHmmPerLane = 4;                                           // B genomes a thread walks its A genome against
constexpr uint32_t kHmmRows = 64;                                             // rows staged per step: one tile of the panel
constexpr uint32_t kHmmRescale = 16;                                          // list positions between two rescales: one dword of codes
constexpr uint32_t kHmmState = 5;                                             // doubles of a pair in the table: F0, F1, V0, V1, E
static_assert(kBlock == 2 * kHmmTile * 4 && kBlock / kHmmTile * kHmmPerLane == kHmmTile && kBlock == 4 * kHmmRows, "k_pair_hmm's thread maps");

typedef double kgx_v2d __attribute__((ext_vector_type(2)));
typedef float kgx_v2f __attribute__((ext_vector_type(2)));

// What the transition of one list position needs: carry, (1 - carry) (1 - pi), (1 - carry) pi, weight.
struct HmmRow { double rho, c0, c1, w; };

// include/kgx.h's class of a called pair of codes: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).
__device__ __forceinline__ uint32_t hmm_class(uint32_t ca, uint32_t cb) {
  const uint32_t x = ca < cb ? ca : cb, y = ca < cb ? cb : ca;
  return 3u * x - x * (x - 1u) / 2u + (y - x);
}

// The table's LDS addresses as integers: entry = of_a + 16 cb in ONE instruction and the row as the read's immediate offset.  (Left to
// itself the compiler merges the two codes first and adds the base after: three instructions a pair and row instead of two.)
typedef const kgx_v2d __attribute__((address_space(3))) * hmm_lds_entry;
__device__ __forceinline__ uint32_t hmm_lds_address(const kgx_v2d* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((hmm_lds_entry)p));
}
__device__ __forceinline__ uint32_t hmm_shift4_add(uint32_t cb, uint32_t base) {
  uint32_t at;
  asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(at) : "v"(cb), "v"(base));
  return at;
}
__device__ __forceinline__ kgx_v2d hmm_entry(uint32_t at, uint32_t offset) {
  return *reinterpret_cast<hmm_lds_entry>(reinterpret_cast<const char __attribute__((address_space(3))) *>(static_cast<uintptr_t>(at)) + offset);
}

// panel: [32 n_tiles genomes or more][panel_pitch], the batch's n_steps = ceil(batch_rows / 64) tiles of 16 bytes; keep: one byte a
// genome, [32 n_tiles], or null; emit: [64 ceil(n_rows / 64)][2][6] and rows: [64 ceil(n_rows / 64)], the WHOLE list's, the
// positions past its end identities; first_row: the batch's first list position, a multiple of 64; state: [G (G + 1) / 2][5];
// result: [G (G + 1) / 2][2]; blockIdx.x: the tile pair, row-major over A <= B.  first_batch: start from {f0, f1, 0, 0}, E = 0;
// last_batch: write the result.
__global__ void __launch_bounds__(kBlock)
k_pair_hmm(const uint8_t* __restrict__ panel, uint64_t panel_pitch, uint32_t n_tiles, uint64_t n_genomes, const uint8_t* __restrict__ keep,
           const float* __restrict__ emit, const HmmRow* __restrict__ rows, uint32_t first_row, uint32_t batch_rows, double f0, double f1,
           bool first_batch, bool last_batch, double* __restrict__ state, double* __restrict__ result) {
  __shared__ kgx_v2d table[2][kHmmRows][16];                                  // [buffer][row][4 ca + cb]: 32 KiB
  __shared__ uint32_t codes[2][4][2 * kHmmTile];                              // [buffer][dword of the tile][genome of A then B]
  uint32_t tile_a = 0, rest = blockIdx.x;
  while (rest >= n_tiles - tile_a) { rest -= n_tiles - tile_a; ++tile_a; }
  const uint32_t tile_b = tile_a + rest;
  const bool diagonal = tile_a == tile_b;
  const uint32_t t = threadIdx.x, n_steps = (batch_rows + kHmmRows - 1u) / kHmmRows;

  // ---- staging: the first 64 threads take a genome's 16 bytes each; every thread takes row t >> 2, code t & 3 of the table
  const uint32_t s_side = t >> 5, s_row = t >> 2, s_ca = t & 3u;
  const bool stages = t < 2u * kHmmTile && !(diagonal && s_side == 1u);
  const uint8_t* src = panel + (static_cast<uint64_t>(s_side == 1u ? tile_b : tile_a) * kHmmTile + (t & 31u)) * panel_pitch;
  kgx_v4u in = {0u, 0u, 0u, 0u};
  kgx_v2f e_in[3];                                                            // {e0, e1} of (ca, cb = 0 .. 2)
  auto fetch = [&](uint32_t step) {
    if (stages) in = *reinterpret_cast<const kgx_v4u*>(src + 16ull * step);
    const float* e = emit + (static_cast<uint64_t>(first_row) + step * kHmmRows + s_row) * 12u;
#pragma unroll
    for (uint32_t cb = 0; cb < 3; ++cb) {
      const uint32_t k = hmm_class(s_ca == 3u ? 0u : s_ca, cb);
      e_in[cb] = kgx_v2f{e[k], e[6u + k]};
    }
  };
  auto stage = [&](uint32_t buffer) {
    if (t < 2u * kHmmTile) {
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) codes[buffer][d][t] = in[d];
    }
    kgx_v2d* entry = &table[buffer][s_row][4u * s_ca];
#pragma unroll
    for (uint32_t cb = 0; cb < 3; ++cb)
      entry[cb] = s_ca == 3u ? kgx_v2d{1.0, 1.0} : kgx_v2d{static_cast<double>(e_in[cb].x), static_cast<double>(e_in[cb].y)};
    entry[3] = kgx_v2d{1.0, 1.0};
  };
  fetch(0u);
  stage(0u);

  // ---- the thread's four pairs
  const uint32_t a_local = t & 31u, b_local = (t >> 5) * kHmmPerLane, b_side = diagonal ? 0u : kHmmTile;
  const uint64_t ga = static_cast<uint64_t>(tile_a) * kHmmTile + a_local, gb0 = static_cast<uint64_t>(tile_b) * kHmmTile + b_local;
  double F0[kHmmPerLane], F1[kHmmPerLane], V0[kHmmPerLane], V1[kHmmPerLane];
  long long E[kHmmPerLane];
  bool stored[kHmmPerLane], walked[kHmmPerLane];                              // a pair of the table; ... both of whose genomes take part
  uint64_t at[kHmmPerLane];
#pragma unroll
  for (uint32_t j = 0; j < kHmmPerLane; ++j) {
    const uint64_t gb = gb0 + j;
    stored[j] = ga < n_genomes && gb < n_genomes && ga <= gb;
    walked[j] = stored[j] && (keep == nullptr || (keep[ga] != 0 && keep[gb] != 0));
    at[j] = stored[j] ? ga * n_genomes - ga * (ga - 1u) / 2u + (gb - ga) : 0u;
    F0[j] = f0; F1[j] = f1; V0[j] = 0.0; V1[j] = 0.0; E[j] = 0;
    if (walked[j] && !first_batch) {
      const double* s = state + kHmmState * at[j];
      F0[j] = s[0]; F1[j] = s[1]; V0[j] = s[2]; V1[j] = s[3]; E[j] = static_cast<long long>(s[4]);
    }
  }
  __syncthreads();

  for (uint32_t step = 0; step < n_steps; ++step) {
    const uint32_t buffer = step & 1u;
    const bool more = step + 1u < n_steps;
    if (more) fetch(step + 1u);
    for (uint32_t g = 0; g < kHmmRows / kHmmRescale; ++g) {
      const uint32_t r0 = step * kHmmRows + g * kHmmRescale;                  // of the batch
      if (r0 >= batch_rows) break;
      const HmmRow* __restrict__ row = rows + (static_cast<uint64_t>(first_row) + r0);
      const uint32_t tb = hmm_lds_address(&table[buffer][g * kHmmRescale][0]);
      const uint32_t aw = codes[buffer][g][a_local];
      uint32_t bw[kHmmPerLane];
#pragma unroll
      for (uint32_t j = 0; j < kHmmPerLane; ++j) bw[j] = codes[buffer][g][b_side + b_local + j];
#pragma unroll
      for (uint32_t r = 0; r < kHmmRescale; ++r) {
        const double rho = row[r].rho, c0 = row[r].c0, c1 = row[r].c1, w = row[r].w;
        const uint32_t of_a = tb + (((aw >> (2u * r)) & 3u) << 6);
#pragma unroll
        for (uint32_t j = 0; j < kHmmPerLane; ++j) {
          const kgx_v2d e = hmm_entry(hmm_shift4_add((bw[j] >> (2u * r)) & 3u, of_a), 256u * r);
          const double S = F0[j] + F1[j], SV = V0[j] + V1[j];
          const double P1 = __builtin_fma(rho, F1[j], c1 * S), P0 = __builtin_fma(rho, F0[j], c0 * S);
          const double Q1 = __builtin_fma(rho, V1[j], c1 * SV), Q0 = __builtin_fma(rho, V0[j], c0 * SV);
          F1[j] = e.y * P1;
          F0[j] = e.x * P0;
          V1[j] = __builtin_fma(e.y, Q1, w * F1[j]);
          V0[j] = e.x * Q0;
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kHmmPerLane; ++j) {                            // F0 + F1 into [1, 2)
        const int k = __builtin_amdgcn_frexp_exp(F0[j] + F1[j]) - 1;
        F0[j] = __builtin_amdgcn_ldexp(F0[j], -k);
        F1[j] = __builtin_amdgcn_ldexp(F1[j], -k);
        V0[j] = __builtin_amdgcn_ldexp(V0[j], -k);
        V1[j] = __builtin_amdgcn_ldexp(V1[j], -k);
        E[j] += k;
      }
    }
    if (more) stage(buffer ^ 1u);
    __syncthreads();                                                          // the other buffer is staged; this one is free
  }

#pragma unroll
  for (uint32_t j = 0; j < kHmmPerLane; ++j) {
    if (!stored[j]) continue;
    double* s = state + kHmmState * at[j];
    s[0] = F0[j]; s[1] = F1[j]; s[2] = V0[j]; s[3] = V1[j]; s[4] = static_cast<double>(E[j]);
    if (!last_batch) continue;
    const double S = F0[j] + F1[j];
    result[2u * at[j]] = walked[j] ? log(S) + static_cast<double>(E[j]) * 0.693147180559945309417232121458 : 0.0;
    result[2u * at[j] + 1u] = walked[j] ? (V0[j] + V1[j]) / S : 0.0;
  }
}

}  // namespace kgx

// The launch shapes and sizes that both the inbreeding kernels (kgx_kernels_common.h, kgx_kernels_inbreed.h, kgx_kernels_hall.h)
// and the host-only plan of a call (kgx_inbreed_plan.h) are built on.  No HIP runtime here: this compiles with a plain C++
// compiler too, and each constant keeps the comment it had beside its kernel.
#ifndef KGX_INBREED_CONSTANTS_H
#define KGX_INBREED_CONSTANTS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define KGX_HOST_DEVICE __host__ __device__
#else
#define KGX_HOST_DEVICE
#endif

namespace kgx {

constexpr int kWave = 64;            // CDNA wavefront
constexpr int kBlock = 256;          // 4 waves per workgroup

// k_inbreed_eval_lut (kgx_kernels_inbreed.h)
constexpr int kEvalBatch = 8;
constexpr uint64_t kRitlandSegment = 4088;        // MODE 3: loci per segment, below the 12-bit class counters' range

// Loglikelihood's searches (k_brent_init, k_brent_step)
constexpr int kSearchBrent = 0, kSearchNelderMead = 1;
constexpr int kSearchNelderMeadPair = 2;

// k_inbreed_iterate_genome
constexpr int kGenomeLoci = 8192;                        // a block per genome: 32 cells per thread; a wave per genome: up to kGenomeWaveLoci
constexpr int kGenomeWaveLoci = 2048;

// The moments (kgx_kernels_hall.h)
constexpr int kHallMoments = 5;                          // M0 (a count) .. M4
constexpr int kHallKeyMantissa = 7;
constexpr int kHallMinExponent = -20;                    // bins reach down to y = 2^-20; below (and above 1) the call takes the 50 passes
constexpr uint32_t kHallBins = 1u + static_cast<uint32_t>(-kHallMinExponent) * (1u << kHallKeyMantissa) + 1u;   // {0}, [2^-20, 1), {1 ..}
constexpr uint32_t kHallItemLoci = 2048;                 // (an item's digit image: 64 KB of the matrix-core pass's LDS; 1024: more items to merge, 4096: one workgroup a CU)
struct HallRecord { uint32_t row; uint32_t bin; double delta; };          // one locus of a class, in bin order: the row it reads, its y = centre(bin) + delta
constexpr uint32_t kHallBlockLoci = 64;                  // (the blocks of slots the class passes walk: see kgx_kernels_hall.h)
// A bit row is cut into SPANS of kBitsSpanGenomes genomes = 256 bytes (k_class_bits)
constexpr uint64_t kBitsSpanGenomes = 2048;
constexpr uint64_t kBitsSpanBytes = kBitsSpanGenomes / 8;
KGX_HOST_DEVICE inline uint64_t hall_bit_row_bytes(uint64_t n_genomes) { return (n_genomes + kBitsSpanGenomes - 1) / kBitsSpanGenomes * kBitsSpanBytes; }

}  // namespace kgx

#endif  // KGX_INBREED_CONSTANTS_H

// Shared by the kernel headers of the C-ABI translation units (gfx950, wave64).
#ifndef KGX_KERNELS_COMMON_H
#define KGX_KERNELS_COMMON_H

#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "kgx_inbreed_constants.h"   // kWave, kBlock and the sizes the host-only plan of an inbreeding call shares with the kernels

typedef uint32_t kgx_v4u __attribute__((ext_vector_type(4)));

#endif  // KGX_KERNELS_COMMON_H

// Device helpers shared by the spectral units (foto_spectral.hip, foto_dct.hip, foto_probe.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace foto {

typedef double dbl4 __attribute__((ext_vector_type(4)));
typedef double dbl2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Write-through 16-B stores (buffer_store_dwordx4 ... sc1): the line leaves the XCD's L2 at
// once instead of staying dirty there.  A streaming kernel that ends with its L2s full of
// dirty lines pays their write-back at the kernel boundary (MI355X_MICROARCH.md price list,
// row "boundary": + B / 6 TB/s for B dirty bytes, up to 32 MiB here).  The resource covers
// [base, base + 2^31 B); offsets are in bytes.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(double* base) {
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void st_wt16(__amdgpu_buffer_rsrc_t rs, int off_bytes, dbl2 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, off_bytes, 0, 16 /* sc1 */);
}

// Loads of a pass's input that is dead after the pass (the DCT chain's intermediates, x^, b^
// in the x^ kernel) are non-temporal: the lines leave the caches first, so the pass's output
// and the next kernel's inputs keep them (A/B against plain loads: DESIGN.md 3.5).
template <class V>
__device__ __forceinline__ V ld_dead(const V* p) {
    return __builtin_nontemporal_load(p);
}

}  // namespace foto

// snarkjs_amd/csrc/fflonk_setup.cuh — the device kernel that the FFLONK setup (src/fflonk_setup.js) adds to those of plonk_setup.cuh.
//
//   k_fsetup_c0   writeC0 (:441-464) and the batchFromMontgomery of CPolynomial.multiExponentiation (src/polynomial/cpolynomial.js:53-83):
//                 C0(X) = QL(X^8) + X QR(X^8) + X^2 QO(X^8) + X^3 QM(X^8) + X^4 QC(X^8) + X^5 S1(X^8) + X^6 S2(X^8) + X^7 S3(X^8).
//                 Thread t = 8 i + j takes coefficient i of polynomial j and writes C0[t] twice: as it is (Montgomery: zkey section 17) and in
//                 canonical form (the scalar of the commitment's MSM). The eight polynomials are read where writeP4 left them: the first
//                 `domain` elements of the eight records (5 x domain elements each: n coefficients, 4n evaluations) in section order
//                 QL QR QM QO QC S1 S2 S3 — so j = 2 reads record 3 and j = 3 reads record 2.
// Both stores are contiguous across the wave (32 bytes a lane); the loads are eight streams, each contiguous across t / 8: a wave reads 8 x 256
// bytes. One Montgomery product a thread, no shared memory, no atomics.
#pragma once
#include "field.cuh"

namespace zkmi {

// recs: 8 records of 5 * domain elements; c0, scalars: 8 * domain elements each
template <class C> __global__ void __launch_bounds__(256)
k_fsetup_c0(const uint32_t* __restrict__ recs, uint32_t* __restrict__ c0, uint32_t* __restrict__ scalars, uint32_t domain) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)8 * domain) return;
    const uint32_t j = (uint32_t)(t & 7);
    const uint32_t rec = j == 2 ? 3u : j == 3 ? 2u : j;                // QO before QM
    const Fp<C> v = fp_load<C>(recs + ((uint64_t)rec * 5 * domain + (t >> 3)) * C::N);
    fp_store<C>(c0 + t * C::N, v);
    fp_store<C>(scalars + t * C::N, fp_from_mont(v));
}

}  // namespace zkmi

// snarkjs_amd/csrc/plonk_setup.cuh — device kernels of the PLONK setup (src/plonk_setup.js) for gfx950.
//
// Everything heavy in a PLONK key runs on kernels the library already has (ntt.hip, the table MSMs, batchApplyKey); these four replace the
// single-threaded loops the reference runs around them:
//   k_psetup_fill      n copies of one element: the ones that zkmi_fr_batch_apply_key_dev turns into power tables.
//   k_psetup_pad       writeQMap (:313-318): the five selector columns of n_rows elements, as the host lowering wrote them, into five
//                      zero-padded domain-sized arrays (the padding never crosses the bus).
//   k_psetup_sigma     writeSigma (:354-422): sigma[p] = ident[pred[p]], ident[col * domain + i] = w^i * {1, k1, k2}[col]. pred[p] is the
//                      position that visited p's signal last before p in the reference's order, or the signal's LAST position for its first
//                      one (the host lowering knows both: plonk_setup.hip). Every position belongs to one signal: every element is written.
//   k_psetup_lagrange  writeLs (:424-434) without its inverse transforms: the ifft of the unit vector e_i is coef_j = w^(-ij) / n, read from
//                      the table pw[e] = w^(-e) / n. Written at the section's record offsets (n coefficients, then room for 4n evaluations).
// Integer only, no atomics, no shared memory; elements are canonical, so a gather leaves the reference's bytes.
#pragma once
#include "field.cuh"

namespace zkmi {

template <class C> __global__ void __launch_bounds__(256) k_psetup_fill(uint32_t* __restrict__ out, uint64_t n, Fp<C> v) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    fp_store<C>(out + i * C::N, v);
}

// in: 5 columns of n_rows elements; out: 5 columns of domain elements
template <class C> __global__ void __launch_bounds__(256)
k_psetup_pad(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n_rows, uint32_t domain) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)5 * domain) return;
    const uint32_t col = (uint32_t)(t / domain), i = (uint32_t)(t % domain);
    const Fp<C> v = i < n_rows ? fp_load<C>(in + ((uint64_t)col * n_rows + i) * C::N) : fp_zero<C>();
    fp_store<C>(out + t * C::N, v);
}

// n = 3 * domain positions; pred[p] < n (checked on the host before the upload)
template <class C> __global__ void __launch_bounds__(256)
k_psetup_sigma(const uint32_t* __restrict__ ident, const uint32_t* __restrict__ pred, uint32_t* __restrict__ sigma, uint64_t n) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    fp_store<C>(sigma + p * C::N, fp_load<C>(ident + (uint64_t)pred[p] * C::N));
}

// polynomial i < n_poly, coefficient j < domain -> out[(i * 5 * domain + j)]
template <class C> __global__ void __launch_bounds__(256)
k_psetup_lagrange(const uint32_t* __restrict__ pw, uint32_t* __restrict__ out, uint32_t n_poly, uint32_t domain) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)n_poly * domain) return;
    const uint64_t i = t / domain, j = t % domain;
    const uint64_t e = (i * j) & (uint64_t)(domain - 1);              // domain is a power of two
    fp_store<C>(out + (i * 5 * domain + j) * C::N, fp_load<C>(pw + e * C::N));
}

}  // namespace zkmi

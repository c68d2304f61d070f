/*
 * include/zkmi.h — C-ABI of the MI355X proving backend (libzkmi.so).
 *
 * This is the drop-in boundary for the snarkjs prover hot path: one entry point per bulk operation
 * that snarkjs issues through ffjavascript's curve object.  Plain pointers and sizes only; the N-API addon
 * (snarkjs_amd/napi/zkmi_napi.c) and the Python ctypes mirror (snarkjs_amd/__init__.py) are thin wrappers.
 * Each declaration cites the reference interface it replaces; `min.js:1@<col>` = column in line 1 of
 * /root/reference/build/snarkjs.min.js (ffjavascript 0.3.1 / wasmcurves 0.2.2 exist in the reference tree only there).
 *
 * Conventions (identical to the reference's in-memory formats):
 *   - field elements: little-endian, n8 bytes (n8r = 32; n8q = 32 BN254 / 48 BLS12-381), Montgomery form unless
 *     stated; scalars handed to the MSM are plain little-endian integers of `scalar_bytes` bytes, NOT reduced mod r.
 *   - affine points (x,y), all-zero bytes = point at infinity; G2 coordinates are (c0,c1) pairs.
 *   - results of MSMs are Jacobian (X,Y,Z), any representative of the group element (snarkjs normalises with
 *     toAffine before serialising); the zero point is returned as all-zero bytes.
 *   - every function returns 0 on success, non-zero on error; zkmi_last_error() describes the last failure on the
 *     calling thread.  Inputs are never modified.  There is NO CPU fallback: without a HIP device every compute
 *     entry point fails with ZKMI_ERR_NO_DEVICE.
 *   - "pages": a logical buffer given as an array of (pointer,length) host segments, because ffjavascript's
 *     BigBuffer (min.js:1@183423) keeps > 1 GiB buffers as a list of <= 1 GiB Uint8Arrays.
 *   - ONE CALLER PER PROCESS. The library keeps one context per process (one process per GPU): the active pipeline slot, its streams
 *     and its scratch buffers are process-global state, and an entry point may swap them while it runs. Calls must therefore be
 *     serialised by the host: the N-API addon takes a mutex around every entry point (main thread and libuv pool threads alike),
 *     the Python mirror a threading.RLock (snarkjs_amd/zkmi.py). zkmi_last_error() is per thread.
 *   - statistics, calibration probes, synthetic-base generators and tuning knobs (no reference counterpart) are declared in
 *     zkmi_diag.h, not here.
 */
#ifndef ZKMI_H
#define ZKMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKMI_CURVE_BN128 0      /* BN254; src/curves.js:9-53 name "bn128" */
#define ZKMI_CURVE_BLS12381 1

#define ZKMI_OK 0
#define ZKMI_ERR_NO_DEVICE 1
#define ZKMI_ERR_INVALID 2
#define ZKMI_ERR_HIP 3
#define ZKMI_ERR_UNSUPPORTED 4

/* Fr batch operations: zkmi_fr_batch(op) */
#define ZKMI_BATCH_TO_MONTGOMERY 0    /* Fr.batchToMontgomery   (helper before min.js:1@185893; src/plonk_prove.js:278) */
#define ZKMI_BATCH_FROM_MONTGOMERY 1  /* Fr.batchFromMontgomery (src/polynomial/polynomial.js:973)                     */
#define ZKMI_BATCH_INVERSE 2          /* Fr.batchInverse        (min.js:1@188677; src/plonk_prove.js:420), 0 -> 0       */

typedef struct zkmi_pages {
    const uint8_t* const* ptr;   /* n_pages segment pointers */
    const size_t* len;           /* n_pages segment lengths in bytes */
    int n_pages;
} zkmi_pages;

/* ---- library / device ------------------------------------------------------------------------------------------- */
/* Bind the calling process to HIP device `device` (>= 0) and create the library context. Idempotent. */
int zkmi_init(int device);
int zkmi_device_count(void);
const char* zkmi_last_error(void);
const char* zkmi_version(void);
/* Use an externally owned hipStream_t for all subsequent launches (NULL = the library's own stream). */
int zkmi_set_stream(void* hip_stream);
/* Block until all work queued by the library has finished. */
int zkmi_synchronize(void);

/* Device memory owned by the library's pool — lets a host without its own HIP binding (the Node addon) keep
 * data resident between calls. */
int zkmi_dev_alloc(size_t bytes, void** d_ptr);
int zkmi_dev_free(void* d_ptr);
int zkmi_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int zkmi_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
/* stream-ordered device-to-device copy / fill on the library stream */
int zkmi_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes);
int zkmi_memset_dev(void* d_dst, int value, size_t bytes);

/* ---- G.multiExpAffine ------------------------------------------------------------------------------------------- */
/* curve.G1.multiExpAffine / curve.G2.multiExpAffine (min.js:1@214996 -> @214651 -> _multiExpChunk @213360; kernel
 * g1m_/g2m_multiexpAffine_chunk @75966).  group = 1 | 2.  n bases of 2*group*n8q bytes, n scalars of scalar_bytes.
 * base_cache_key & ZKMI_BASES_CACHE ALLOWS the library to keep these bases resident (zkey sections / SRS slices are static per circuit,
 * src/groth16_prove.js:84-100); its value carries no identity. The cache is content-addressed: the library hashes the whole base
 * buffer on every call (128 bits per 64 KiB chunk, a fast NON-cryptographic mix: accidental changes — another zkey, an edited section —
 * are told apart, deliberately constructed colliding buffers are not; callers that take bases from an untrusted party pass key 0). The
 * pre-computed window table of a buffer is built on its SECOND sight, an MSM over a prefix of a resident buffer re-uses its
 * table, tables that cannot fit are never built (plain bases instead), and least-recently-used tables are evicted under a
 * byte budget (env ZKMI_BASE_CACHE_BYTES, default 64 GiB). zkmi_release_bases drops every cached table.
 * base_cache_key is a set of permission bits (any other bit is ignored):
 *   ZKMI_BASES_CACHE (1)      resident tables allowed; identity = the FULL content hash, on every call: the result is always a function of the
 *                             bytes passed, like the reference's (min.js:1@213360) — an in-place edit of a resident buffer is seen by the next call.
 *   ZKMI_BASES_IMMUTABLE (2)  (with bit 1) the caller PROMISES that a buffer it passes again at the same first-page address with the same length
 *                             still holds the same bytes (a zkey section it never writes to). Only then a buffer that has been checked byte for
 *                             byte against a resident table is re-checked by SAMPLE (its first and last whole chunk and 30 chunks at positions that
 *                             change from call to call; 2 MB instead of 64 MB hashed at 2^20 points) and in full on every 32nd sight. A caller that
 *                             breaks the promise can be handed the old buffer's result for up to 31 calls. Never assumed by default (r04 did; r05:
 *                             opt-in): register(curve, {immutableBases: true}) in js/register.js, cache_key=3 in the Python mirror.
 * ZKMI_BASE_HASH_FULL=1 in the environment forces the full hash whatever the caller promised.
 * out_jacobian: 3*group*n8q bytes. */
#define ZKMI_BASES_CACHE 1ull
#define ZKMI_BASES_IMMUTABLE 2ull
int zkmi_msm(int curve, int group, zkmi_pages bases, zkmi_pages scalars, size_t n, size_t scalar_bytes,
             uint64_t base_cache_key, uint8_t* out_jacobian);
int zkmi_release_bases(uint64_t base_cache_key);
/* Same with bases and scalars already resident in device memory (bench.py, fused pipelines). */
int zkmi_msm_dev(int curve, int group, const void* d_bases, const void* d_scalars, size_t n, size_t scalar_bytes,
                 uint8_t* out_jacobian);
/* Resident bases with pre-computed window tables T[k][i] = 2^(c*k) * P_i (static per zkey / SRS: src/groth16_prove.js:84-100,
 * src/polynomial/polynomial.js:970-977 slices the same PTau for every commitment). Build once from n device-resident affine
 * points; each MSM then uses the first k <= n bases with k scalars of at most 32 bytes. */
int zkmi_msm_table_build(int curve, int group, const void* d_bases, size_t n, uint64_t* handle);
int zkmi_msm_table_dev(uint64_t handle, const void* d_scalars, size_t k, size_t scalar_bytes, uint8_t* out_jacobian);
/* up to 4 independent MSMs against one table in a single call (PLONK commits A,B,C / T1,T2,T3 / Wxi,Wxiw per round): their
 * latency-bound bucket reductions share one set of launches. out_jacobians: count x 3*group*n8q bytes. */
int zkmi_msm_table_multi_dev(uint64_t handle, const void* const* d_scalars, const size_t* ks, int count, size_t scalar_bytes,
                             uint8_t* out_jacobians);
/* The same call in two halves (r06), for a host that drives two proofs from one thread (zkmi_pipeline_select): _enqueue_dev puts the digit sorts, accumulations and bucket
 * reductions of the MSMs on the ACTIVE pipeline slot's streams and returns at once; _collect (same slot, same table, same count) waits for them, folds the window sums and writes
 * count x 3*group*n8q bytes. Between the two the host can enqueue the other proof's work — its accumulations then run underneath this call's latency-bound reduction tail.
 * d_scalars must stay valid until the collect; one enqueued call per pipeline slot (an enqueued call that is never collected — its proof was abandoned — is waited for and
 * dropped by the slot's next enqueue).
 * Between the two halves the call's window sums sit in pinned host memory of the slot, and the collect folds whatever is there. Every other entry point that uses that
 * memory in the same slot is therefore REFUSED until the collect (ZKMI_ERR_INVALID, "<entry>: pipeline slot N holds work in flight (collect it first)"): see the rule at
 * zkmi_pipeline_select below. Transforms, Fr batch operations, the zkmi_poly_* calls, zkmi_to_affine and the batch verifiers take none of it and stay allowed. */
int zkmi_msm_table_multi_enqueue_dev(uint64_t handle, const void* const* d_scalars, const size_t* ks, int count, size_t scalar_bytes);
int zkmi_msm_table_multi_collect(uint64_t handle, int count, uint8_t* out_jacobians);
/* Polynomial.multiExponentiation (src/polynomial/polynomial.js:970-977) for the commitments of one round: the `count` coefficient arrays are MONTGOMERY Fr elements; their
 * batchFromMontgomery (one launch for all of them, into scratch memory of the active pipeline slot) and the MSMs are enqueued as by zkmi_msm_table_multi_enqueue_dev. The
 * polynomials are read by the conversion launch only, which is stream-ordered before anything the caller enqueues on the slot afterwards. Collect with zkmi_msm_table_multi_collect. */
int zkmi_msm_table_multi_enqueue_mont_dev(uint64_t handle, const void* const* d_polys, const size_t* ks, int count);
int zkmi_msm_table_release(uint64_t handle);
/* Curve, group and number of resident points of a table (any pointer may be NULL): a binding sizes the result buffers of the two calls above
 * — 3*group*n8q bytes per MSM — from the TABLE instead of trusting its caller. */
int zkmi_msm_table_info(uint64_t handle, int* curve, int* group, size_t* n);

/* ---- Fr.fft / Fr.ifft ------------------------------------------------------------------------------------------- */
/* curve.Fr.fft / curve.Fr.ifft (min.js:1@215859; kernels frm_fftMix/_fftJoin/_fftFinal @103755):
 *   X[k] = sum_j x[j] w^(jk), w = Fr.w[log_n], natural order in and out; inverse includes the 1/n scaling.
 * n = 2^log_n elements of 32 bytes; log_n must be <= Fr.s (28 BN254, 32 BLS12-381) — the reference's extra
 * n = 2^(s+1) coset case (@216148) is rejected with ZKMI_ERR_UNSUPPORTED.
 * Sizes above 2^24 run four passes over the array instead of at most three; they are tested at 2^25 / 2^26 (tests/test_gpu_ntt_passes.py).
 * Optional fused pre-scale x[i] <- x[i]*first*inc^i (= Fr.batchApplyKey in front, src/groth16_prove.js:66-76):
 * pass prescale_first = prescale_inc = NULL for a plain transform. */
int zkmi_ntt(int curve, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, unsigned log_n,
             int inverse, const uint8_t* prescale_first, const uint8_t* prescale_inc);
int zkmi_ntt_dev(int curve, const void* d_in, void* d_out, unsigned log_n, int inverse, const uint8_t* prescale_first,
                 const uint8_t* prescale_inc);
/* Evaluations.fromPolynomial (src/polynomial/evaluations.js:30-37): the transform of a polynomial of in_len <= 2^log_n coefficients, zero-padded to 2^log_n — the padding is
 * never written: the first pass reads zeros beyond in_len. d_out: 2^log_n elements (d_in == d_out allowed when that buffer is 2^log_n long). */
int zkmi_ntt_padded_dev(int curve, const void* d_in, size_t in_len, void* d_out, unsigned log_n, int inverse);

/* ---- Fr batch operations ---------------------------------------------------------------------------------------- */
/* curve.Fr.batchApplyKey(buf, first, inc) (min.js:1@211529, kernel frm_batchApplyKey @128060): out[i] = in[i]*first*inc^i */
int zkmi_fr_batch_apply_key(int curve, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages,
                            size_t n, const uint8_t* first, const uint8_t* inc);
int zkmi_fr_batch_apply_key_dev(int curve, const void* d_in, void* d_out, size_t n, const uint8_t* first, const uint8_t* inc);
/* op = ZKMI_BATCH_* */
int zkmi_fr_batch(int curve, int op, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, size_t n);
int zkmi_fr_batch_dev(int curve, int op, const void* d_in, void* d_out, size_t n);
/* the two Montgomery conversions on up to four arrays in one launch (ns[i] elements each; in place allowed) */
int zkmi_fr_batch_multi_dev(int curve, int op, const void* const* d_in, void* const* d_out, const size_t* ns, int count);
/* joinABC (src/groth16_prove.js:320-374: qap_joinABC min.js:1@123664 + frm_batchFromMontgomery):
 * out[i] = fromMontgomery(a[i]*b[i] - c[i]) */
int zkmi_groth16_join_abc(int curve, zkmi_pages a, zkmi_pages b, zkmi_pages c, uint8_t* const* out_ptr,
                          const size_t* out_len, int n_out_pages, size_t n);
int zkmi_groth16_join_abc_dev(int curve, const void* d_a, const void* d_b, const void* d_c, void* d_out, size_t n);

/* ---- fused Groth16 prover ---------------------------------------------------------------------- */
/* groth16Prove (src/groth16_prove.js:28-144) from already-read sections: buildABC1 (:147-187) as a device kernel,
 * 3 x (ifft -> coset scale -> fft), joinABC, 4 G1 MSMs + 1 G2 MSM, blinding (:103-120) and toAffine (:130-132).
 * All section pointers are HOST pointers in the zkey/wtns on-disk layout (src/zkey_utils.js:229-259):
 *   coeffs = zkey section 4; bases_a/b1/c/h = sections 5,6,8,9 (G1 affine); bases_b2 = section 7 (G2 affine);
 *   witness = wtns section 2 (n_vars x 32 B, normal form); vk_* = header points (affine);
 *   r_mont / s_mont = the two Fr.random() draws (:103-104), Montgomery form.
 * zkey_cache_key != 0 keeps the five base tables and the coefficient table resident across calls.
 * Outputs are affine Montgomery: pi_a, pi_c 2*n8q bytes, pi_b 4*n8q bytes. */
typedef struct zkmi_groth16_zkey {
    int curve;
    uint32_t n_vars, n_public, domain_size;
    const uint8_t* coeffs; size_t coeffs_len;
    const uint8_t *bases_a, *bases_b1, *bases_b2, *bases_c, *bases_h;
    const uint8_t *vk_alpha_1, *vk_beta_1, *vk_beta_2, *vk_delta_1, *vk_delta_2;
    /* byte lengths of sections 5, 6, 7, 8, 9 as found in the file: checked against nVars / nPublic / domainSize of the header before
     * anything is read (a truncated or malformed zkey fails with ZKMI_ERR_INVALID instead of reading past the caller's buffers; the
     * reference gets the same protection from bounds-checked JS buffers). The vk_* points are 2*n8q (G1) / 4*n8q (G2) bytes. */
    size_t bases_a_len, bases_b1_len, bases_b2_len, bases_c_len, bases_h_len;
} zkmi_groth16_zkey;
/* Upload the proving key under `zkey_cache_key` (!= 0): base tables + the coefficient section as a length-sorted sliced layout. */
int zkmi_groth16_load(const zkmi_groth16_zkey* zkey, uint64_t zkey_cache_key);
/* The same with every bulk section given as PAGES: what the reference holds after binFileUtils.readSection (src/groth16_prove.js:29-33, :57-59,
 * :84-100) — a Uint8Array below 2^30 bytes, a BigBuffer of <= 1 GiB pages from there on (sections 4-9 of a 2^24-constraint key are 1 - 2 GB
 * each; one Node buffer ends at 2 GiB - 1). Section lengths are the page totals; they are checked against the header like the flat form's.
 * A page whose POINTER is NULL is a gap of `len` bytes the caller did not read: zkmi_groth16_load_shard_paged only touches the byte ranges of
 * its own variables / H bases, so a shard process reads just those from the file (js/groth16_shards.js) and passes the rest as gaps; a load
 * that needs a byte inside a gap fails with ZKMI_ERR_INVALID. The coefficient section is needed whole by every loader. */
typedef struct zkmi_groth16_zkey_paged {
    int curve;
    uint32_t n_vars, n_public, domain_size;
    zkmi_pages coeffs, bases_a, bases_b1, bases_b2, bases_c, bases_h;      /* zkey sections 4, 5, 6, 7, 8, 9 */
    const uint8_t *vk_alpha_1, *vk_beta_1, *vk_beta_2, *vk_delta_1, *vk_delta_2;
} zkmi_groth16_zkey_paged;
int zkmi_groth16_load_paged(const zkmi_groth16_zkey_paged* zkey, uint64_t zkey_cache_key);
int zkmi_groth16_load_shard_paged(const zkmi_groth16_zkey_paged* zkey, uint64_t zkey_cache_key, uint32_t var_lo, uint32_t var_hi, uint32_t h_lo, uint32_t h_hi);
/* zkmi_groth16_prove (below) with the paged descriptor: same key semantics (load on first use, descriptor checked against a resident key, key 0 =
 * load, prove, release). */
int zkmi_groth16_prove_paged(const zkmi_groth16_zkey_paged* zkey, uint64_t zkey_cache_key, const uint8_t* witness, size_t witness_len,
                             const uint8_t* r_mont, const uint8_t* s_mont, uint8_t* pi_a, uint8_t* pi_b, uint8_t* pi_c);
/* buildABC1 (src/groth16_prove.js:147-187) alone, on a resident key: A_T, B_T, C_T = A_T * B_T (domain x 32 bytes each, Montgomery) from the
 * witness in device memory (normal form); any output may be NULL. Rows are balanced by length: a 10^5-term row of a real circuit is spread
 * over thousands of lanes (csrc/groth16.hip). zkmi_last_kernel_ms() = the device time of the three kernels. */
int zkmi_groth16_build_abc_dev(uint64_t zkey_cache_key, const void* d_witness, void* d_a, void* d_b, void* d_c);
/* One proof. zkey_cache_key != 0: the key is loaded on first use (zkey may be NULL afterwards) and stays resident; a descriptor
 * given together with an already resident key must describe the same circuit (curve, nVars, nPublic, domainSize, nCoef), else the
 * call fails with ZKMI_ERR_INVALID — release the key first to replace it. zkey_cache_key == 0: load, prove, release.
 * `witness` is a HOST pointer to wtns section 2 (normal form), witness_len its byte length: must be n_vars x 32
 * ("Invalid witness length", src/groth16_prove.js:45-47). */
int zkmi_groth16_prove(const zkmi_groth16_zkey* zkey, uint64_t zkey_cache_key, const uint8_t* witness, size_t witness_len,
                       const uint8_t* r_mont, const uint8_t* s_mont, uint8_t* pi_a, uint8_t* pi_b, uint8_t* pi_c);
/* Same with the witness already in device memory and the key loaded (bench.py: inputs resident in HBM). */
int zkmi_groth16_prove_dev(uint64_t zkey_cache_key, const void* d_witness, const uint8_t* r_mont, const uint8_t* s_mont,
                           uint8_t* pi_a, uint8_t* pi_b, uint8_t* pi_c);
/* Two proofs in flight on one GPU (throughput mode): zkmi_groth16_submit_dev enqueues the whole device part of a proof into
 * pipeline slot 0 or 1 and returns at once; zkmi_groth16_collect waits for that slot, folds the window sums and applies the
 * blinding + toAffine. While proof k sits in its latency-bound tail (bucket reductions: few waves, long dependency chains; result
 * copies; host folds) the throughput-bound front of proof k+1 (buildABC, NTTs, accumulations) already runs. Each slot owns its
 * streams, scratch and work buffers; d_witness must stay valid until the slot is collected. prove_dev == submit(0) + collect(0). */
int zkmi_groth16_submit_dev(uint64_t zkey_cache_key, const void* d_witness, int slot);
/* Host-orchestrated provers (plonk.prove, fflonk.prove: the rounds are driven by the host between transcript hashes) with two proofs in flight
 * from ONE host thread: every library call works on the ACTIVE pipeline slot (0 | 1) — its own stream and events, scratch buffers, pool of
 * zkmi_dev_alloc blocks and ring of per-call constants — so the host alternates between two proofs, switching slots at its blocking calls, and
 * the GPU always holds the queued work of the other proof (snarkjs_amd/plonk.py: prove_many). Resident keys and window tables are shared.
 *
 * ONE USER OF A SLOT'S MSM RESULTS AT A TIME. A slot HOLDS WORK IN FLIGHT from zkmi_msm_table_multi_enqueue(_mont)_dev to its zkmi_msm_table_multi_collect, from
 * zkmi_groth16_submit(_dev) to its zkmi_groth16_collect, and from zkmi_groth16_sums_w_dev to the zkmi_groth16_sums_h_dev that completes it. The per-window sums of that work
 * land in pinned host memory owned by the slot and are folded by the collect, so while a slot holds work in flight every OTHER entry point that computes an MSM in it fails
 * with ZKMI_ERR_INVALID and "<entry>: pipeline slot N holds work in flight (collect it first)" before it touches the slot's pinned sums (the Groth16 entry points before
 * they enqueue anything at all; zkmi_msm and zkmi_msm_dev may already have staged their bases in scratch of their own, stream-ordered behind the work in flight): zkmi_msm, zkmi_msm_dev, zkmi_msm_table_dev,
 * zkmi_msm_table_multi_dev, a multi-MSM enqueue over a Groth16 proof, and every Groth16 proof (zkmi_groth16_prove*, _submit*, _sums_*) over an enqueued multi-MSM call or over
 * a proof of ANOTHER resident key (a second submit of the same key keeps its own message). The work in flight is not disturbed by the refused call and collects to its exact
 * result. Not refused: the collects themselves; an enqueue over this slot's own enqueued multi-MSM call (dropped as abandoned, see above); anything in the OTHER slot;
 * and everything that computes no MSM (zkmi_ntt*, zkmi_fr_batch*, zkmi_poly_*, zkmi_plonk_* / zkmi_fflonk_* round kernels, zkmi_to_affine, the batch verifiers): the slot's
 * stream orders their scratch behind the work in flight. zkmi_groth16_prove with a host witness always runs in slot 0, whichever slot is active. The three setups ask for
 * BOTH slots to be idle. */
int zkmi_pipeline_select(int slot);
int zkmi_pipeline_active(void);
/* The same for a witness in HOST memory (wtns section 2, witness_len = n_vars x 32): it crosses PCIe on the slot's own stream into the
 * slot's own buffer, i.e. underneath the kernels of the proof in the other slot — the throughput mode of a host that keeps witnesses in
 * host memory (js/groth16_native.js: proveMany). `witness` may be re-used as soon as the call returns. */
int zkmi_groth16_submit(uint64_t zkey_cache_key, const uint8_t* witness, size_t witness_len, int slot);
int zkmi_groth16_collect(uint64_t zkey_cache_key, int slot, const uint8_t* r_mont, const uint8_t* s_mont, uint8_t* pi_a, uint8_t* pi_b, uint8_t* pi_c);
int zkmi_groth16_release(uint64_t zkey_cache_key);
/* ---- Groth16 setup: zKey.newZKey (src/zkey_new.js) ------------------------------------------------------------------
 * The device part of newZKey from already-read slices: processConstraints (:203-336), composeAndWritePoints for sections 3, 8, 5, 6, 7
 * (:338-502, task lists the reference sends straight to its workers: no curve method sees them) and the H points of hashHPoints (:504-577).
 *   constraints        r1cs section 2 as it lies in the file: per constraint three linear combinations, each u32 n then n x (u32 signal, 32-byte
 *                      little-endian coefficient). Parsed on the host side of the library in one pass.
 *   tau_g1 .. beta_tau_g1   the domain_size Lagrange points that start at offset (domain_size - 1) * sG of ptau sections 12, 13, 14, 15.
 *   tau_g1_powers      the first domain_size + n_h points of ptau section 2; n_h = number of H points the reference hashes: domain_size - 1, or
 *                      domain_size for domains of 2^15 and above (the chunk loop of :509-513 takes one point more there).
 * Outputs (caller-owned, lengths checked): ic = section 3 ((n_public + 1) G1), coeffs = section 4 (length from zkmi_groth16_setup_coeffs_len:
 * records in constraint order, A entries before B entries, then the binding rows, values times R^2 mod r), a, b1 = sections 5, 6 (n_vars G1),
 * b2 = section 7 (n_vars G2), c = section 8 ((n_vars - n_public - 1) G1): affine Montgomery little-endian, a signal absent from a matrix = all-zero
 * bytes; h = the n_h differences tauG1[i + domain_size] - tauG1[i], affine, UNCOMPRESSED (big-endian normal form) as they enter the circuit hash.
 * Fails with ZKMI_ERR_INVALID when a pipeline slot holds work in flight (it uses the active slot's stream). */
typedef struct zkmi_groth16_setup_in {
    int curve;
    uint32_t n_constraints, n_vars, n_public, domain_size, n_h;
    zkmi_pages constraints, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, tau_g1_powers;
} zkmi_groth16_setup_in;
typedef struct zkmi_groth16_setup_out {
    uint8_t *ic, *coeffs, *a, *b1, *b2, *c, *h;
    size_t ic_len, coeffs_len, a_len, b1_len, b2_len, c_len, h_len;
} zkmi_groth16_setup_out;
/* byte length of section 4 for these constraints; host only, needs no device */
int zkmi_groth16_setup_coeffs_len(zkmi_pages constraints, uint32_t n_constraints, uint32_t n_public, size_t* len);
/* section 4 alone (processConstraints, :303-334), out_len as returned above; host only, needs no device */
int zkmi_groth16_setup_coeffs(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint8_t* out, size_t out_len);
int zkmi_groth16_setup(const zkmi_groth16_setup_in* in, const zkmi_groth16_setup_out* out);
/* ---- PLONK setup: plonk.setup (src/plonk_setup.js) ---------------------------------------------------------------------
 * Two steps, because the size of everything depends on the gate lowering. (1) zkmi_plonk_setup_lower, host only, needs no device:
 * processConstraints (:143-302) as one serial pass over r1cs section 2 (`constraints`, as it lies in the file; n_constraints, n_vars, n_public from
 * the r1cs header). zkmi_plonk_setup_lower_len returns counts4 = plonkNVars, the number of additions, the number of PLONK constraints and domainSize
 * (2^max(3, log2(constraints - 1) + 1), the reference's log2); the caller puts them into a zkmi_plonk_lowered with buffers of
 *   additions   n_additions x 72 bytes: zkey section 3 (u32 signal, u32 signal, two Montgomery factors),
 *   map_a/b/c   n_constraints x u32: sections 4, 5, 6,
 *   selectors   Qm | Ql | Qr | Qo | Qc, five columns of n_constraints x 32 bytes, Montgomery (what writeQMap :313-318 puts into its buffer),
 *   pred        3 x domain_size x u32: for position p = column * domain_size + row of the permutation, the position whose value writeSigma
 *               (:354-422) stores at p: the one that visited p's signal last before p, or the signal's last position for its first one,
 * and zkmi_plonk_setup_lower fills them (ZKMI_ERR_INVALID when the counts are not those of the constraints). The reference's reading of an r1cs is
 * kept: one coefficient per signal and linear combination (the last in the file), keys in ascending order, zero coefficients stay.
 * (2) zkmi_plonk_setup, on the device: lagrange_g1 = the domain_size points that start at offset (domain_size - 1) * sG1 of ptau section 12.
 * Outputs (caller-owned, lengths checked): q[0..5) = sections 7 - 11 (Qm Ql Qr Qo Qc), each n coefficients then 4n evaluations (writeP4 :326-333,
 * q_len = 5 n x 32); sigma = section 12 (three such records); lagrange = section 13 (max(n_public, 1) records); commitments = Qm Ql Qr Qo Qc S1
 * S2 S3 as the header holds them, affine Montgomery, infinity = all-zero bytes. k1 = 2, k2 = 3 (getK1K2 :484-504 cannot return anything else).
 * Fails with ZKMI_ERR_INVALID when a pipeline slot holds work in flight (it uses the active slot's stream). */
typedef struct zkmi_plonk_lowered {
    uint32_t plonk_n_vars, n_additions, n_constraints, domain_size;
    uint8_t* additions;
    uint32_t *map_a, *map_b, *map_c;
    uint8_t* selectors;
    uint32_t* pred;
} zkmi_plonk_lowered;
int zkmi_plonk_setup_lower_len(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint32_t* counts4);
int zkmi_plonk_setup_lower(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, const zkmi_plonk_lowered* out);
typedef struct zkmi_plonk_setup_in {
    int curve;
    uint32_t n_public, n_constraints, domain_size;      /* n_constraints: PLONK constraints (rows of the selector columns) */
    const uint8_t* selectors;
    const uint32_t* pred;
    zkmi_pages lagrange_g1;
} zkmi_plonk_setup_in;
typedef struct zkmi_plonk_setup_out {
    uint8_t* q[5];
    uint8_t *sigma, *lagrange, *commitments;
    size_t q_len, sigma_len, lagrange_len, commitments_len;
} zkmi_plonk_setup_out;
int zkmi_plonk_setup(const zkmi_plonk_setup_in* in, const zkmi_plonk_setup_out* out);
/* ---- FFLONK setup: fflonk.setup (src/fflonk_setup.js), BN254 -----------------------------------------------------------
 * The same two steps. (1) zkmi_fflonk_setup_lower, host only, needs no device: computeFFConstraints (:160-209) through
 * src/r1cs_constraint_processor.js as one serial pass. It fills a zkmi_plonk_lowered (plonk_n_vars = the header's nVars after the lowering), with
 * these differences: selectors are QL | QR | QM | QO | QC (sections 7 - 11 in that order); zero coefficients leave a combination before it is
 * classified and after a join; zkmi_fflonk_setup_lower_len's domainSize is 2^max(3, log2(constraints + 1) + 1), which keeps two rows free; in pred
 * the rows from the constraint count up to domain_size - 3 hold signal 0 and the last two rows point at themselves (the identity, :356-359).
 * (2) zkmi_fflonk_setup, on the device: tau_g1 = the first 8 * domain_size points of ptau section 2. Outputs (caller-owned, lengths checked):
 * q[0..5) = sections 7 - 11, sigma = sections 12, 13, 14 one after the other, each record n coefficients then 4n evaluations (q_len = 5 n x 32,
 * sigma_len = 15 n x 32); lagrange = section 15 (max(n_public, 1) records); c0 = section 17 (8 n x 32: coefficient i of QL QR QO QM QC S1 S2 S3 at
 * 8 i + j, Montgomery); commitment = [C0]_1 of the header, affine Montgomery. k1 = 2, k2 = 3 (computeK1K2 :513-532 cannot return anything else).
 * ZKMI_ERR_UNSUPPORTED for BLS12-381 (all three entries: the reference writes BN254's w3 and wr into such a key, so no proof under it verifies) and
 * for domains above 2^26; ZKMI_ERR_INVALID when a pipeline slot holds work in flight (it uses the active slot's stream). */
int zkmi_fflonk_setup_lower_len(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, uint32_t* counts4);
int zkmi_fflonk_setup_lower(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint32_t n_public, const zkmi_plonk_lowered* out);
typedef struct zkmi_fflonk_setup_in {
    int curve;
    uint32_t n_public, n_constraints, domain_size;      /* n_constraints: rows of the selector columns */
    const uint8_t* selectors;
    const uint32_t* pred;
    zkmi_pages tau_g1;
} zkmi_fflonk_setup_in;
typedef struct zkmi_fflonk_setup_out {
    uint8_t* q[5];
    uint8_t *sigma, *lagrange, *c0, *commitment;
    size_t q_len, sigma_len, lagrange_len, c0_len, commitment_len;
} zkmi_fflonk_setup_out;
int zkmi_fflonk_setup(const zkmi_fflonk_setup_in* in, const zkmi_fflonk_setup_out* out);
/* groth16Verify (src/groth16_verify.js:26-87) for batches of proofs against one verifying key, on the device, one verdict per proof.
 * zkmi_groth16_vk_load takes the key's points as the reference's fromObject reads them: (x, y, z) triples in standard form, little-endian,
 * n8q bytes per Fq (Fq2 = c0 | c1); z = 0 infinity, z = 1 affine, other z Jacobian. ic_xyz holds nPublic + 1 points (IC[0..nPublic]).
 * zkmi_groth16_verify_batch: proofs_xyz = n records pi_a (3 Fq) | pi_b (3 Fq2) | pi_c (3 Fq); publics = n x n_signals x 32 bytes,
 * little-endian integers (the first n_signals IC points are used; n_signals > nPublic is an error, where the reference throws).
 * verdicts[i]: 1 valid ("OK!"), 0 pairing check failed ("Invalid proof"), -1 a public input >= r ("Public inputs are not valid."),
 * -2 a proof point not on the curve ("Proof commitments are not valid."). The verifier has its own stream and buffers: it never
 * touches the pipeline slots of the provers. */
int zkmi_groth16_vk_load(int curve, const uint8_t* alpha1_xyz, const uint8_t* beta2_xyz, const uint8_t* gamma2_xyz, const uint8_t* delta2_xyz,
                         const uint8_t* ic_xyz, uint32_t n_public, uint64_t* vk_handle);
int zkmi_groth16_verify_batch(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts);
int zkmi_groth16_vk_release(uint64_t vk_handle);
/* plonkVerify (src/plonk_verify.js:29-123) for batches of proofs against one verifying key, on the device, one verdict per proof; same
 * conventions as the Groth16 trio above (standard form, little-endian, (x, y, z) triples). zkmi_plonk_vk_load: g1_points_xyz = Qm Ql Qr Qo Qc
 * S1 S2 S3 (3 Fq each), x2_xyz = X_2 (3 Fq2), k1 / k2 32 bytes each; a key point off its curve is refused. zkmi_plonk_verify_batch: proofs = n
 * records A B C Z T1 T2 T3 Wxi Wxiw (3 Fq each) | eval_a eval_b eval_c eval_s1 eval_s2 eval_zw (32 bytes each, reduced modulo r as
 * Fr.fromObject does); publics = n x n_signals x 32 bytes. n_signals != nPublic is refused for the whole call with the reference's message
 * "Invalid number of public inputs" (code -3 of the wrappers). verdicts[i]: 1 valid ("OK!"), 0 pairing check failed ("Invalid Proof"),
 * -2 a commitment not on the curve ("Proof commitments are not valid."), -1 a public input >= r ("Public inputs are not valid."), checked in
 * that order; -4 ("Proof evaluations are not valid") is reserved: the reference's test cannot fire. The verifier has a stream, buffers and a
 * lock of its own: it never touches the pipeline slots of the provers or the Groth16 verifier. */
int zkmi_plonk_vk_load(int curve, const uint8_t* g1_points_xyz, const uint8_t* x2_xyz, const uint8_t* k1, const uint8_t* k2, uint32_t power, uint32_t n_public,
                       uint64_t* vk_handle);
int zkmi_plonk_verify_batch(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts);
int zkmi_plonk_vk_release(uint64_t vk_handle);
/* The curve (ZKMI_CURVE_*) and nPublic of a loaded PLONK verifying key, so that a caller can size a batch's buffers: a record is 27 n8q + 192 bytes. */
int zkmi_plonk_vk_info(uint64_t vk_handle, int* curve, uint32_t* n_public);
/* fflonkVerify (src/fflonk_verify.js:28-137) for batches of proofs against one verifying key, on the device, one verdict per proof; same
 * conventions as the PLONK calls above. BN254 only: ZKMI_CURVE_BLS12381 is refused (the reference has no FFLONK on that curve). zkmi_fflonk_vk_load:
 * c0_xyz = C0 (3 Fq), x2_xyz = X_2 (3 Fq2), consts = k1 k2 w3 w4 w8 wr (32 bytes each, standard form); w is Fr.w[power]. An X_2 off its curve
 * is refused; a C0 off the curve loads, and every proof under that key gets -2, as the reference has it. zkmi_fflonk_verify_batch: proofs = n
 * records C1 C2 W1 W2 (3 Fq each) | ql qr qm qo qc s1 s2 s3 a b c z zw t1w t2w (32 bytes each, reduced modulo r as Fr.fromObject does; the
 * proof's `inv` is not read): 12 n8q + 480 bytes; publics = n x n_signals x 32 bytes. The reference tests the number of signals FIRST:
 * n_signals != nPublic is refused for the whole call with its message "Number of public signals does not match with vk" (code -3 of the
 * wrappers, for every proof of the call whatever its commitments are). verdicts[i]: -2 a commitment (or C0) not on the curve ("Proof commitments are not valid"), -1 a
 * public input >= r ("Public inputs are not valid."), checked in that order, then 0 pairing check failed ("Invalid Proof") or 1 valid
 * ("PROOF VERIFIED SUCCESSFULLY"); -4 ("Proof evaluations are not valid.") is reserved: the reference's test cannot fire. The verifier has a
 * stream, buffers and a lock of its own: it never touches the pipeline slots of the provers or the other verifiers. */
int zkmi_fflonk_vk_load(int curve, const uint8_t* c0_xyz, const uint8_t* x2_xyz, const uint8_t* consts, uint32_t power, uint32_t n_public, uint64_t* vk_handle);
int zkmi_fflonk_verify_batch(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, int8_t* verdicts);
int zkmi_fflonk_vk_release(uint64_t vk_handle);
/* The curve (ZKMI_CURVE_*) and nPublic of a loaded FFLONK verifying key, so that a caller can size a batch's buffers. */
int zkmi_fflonk_vk_info(uint64_t vk_handle, int* curve, uint32_t* n_public);
/* The aggregated check of a batch under one PLONK / FFLONK key: "are ALL of these valid?" by ONE pairing check. Inputs and refusals
 * as zkmi_*_verify_batch; seed = 32 bytes the maker of the proofs could not predict. r_i = the first 16 bytes, little-endian, of
 * Keccak-256(seed | LE64(i)) with bit 127 set; codes[i] = the input checks' code of proof i (-2 / -1 as above) or 1: its pair entered the sums
 * S_P = sum r_i P_i, S_Q = sum r_i Q_i; *ok = 1 exactly when every code is 1 and e(-S_P, T0) e(S_Q, T1) == 1 (PLONK: A1, B1, X_2, [1]_2; FFLONK: A1,
 * W2, [1]_2, X_2). An empty batch is ok. If every per-proof verdict is 1, ok is 1; if one is not, ok is 0 except with probability about 2^-127
 * over the seed (proof points in G1; on BLS12-381 the sums are multiplied by the G1 cofactor first, so a point outside G1 enters through its G1
 * component only). */
int zkmi_plonk_verify_aggregate(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                int* ok);
int zkmi_fflonk_verify_aggregate(uint64_t vk_handle, const uint8_t* proofs, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                 int* ok);
/* The aggregated check of a batch under one Groth16 key: "are ALL of these valid?" by ONE final exponentiation. Records and refusals
 * as zkmi_groth16_verify_batch (n_signals below nPublic is accepted, above is refused); seed and r_i as above. codes[i] = the input checks' code of
 * proof i (-1 / -2) or 1: it entered F = prod Miller(-r_i A_i, B_i), S_X = sum r_i vk_x_i, S_C = sum r_i C_i and s = sum r_i; *ok = 1 exactly when
 * every code is 1 and F e(S_X, gamma) e(S_C, delta) e(alpha, beta)^s reduces to 1. An empty batch is ok. If every per-proof verdict is 1, ok is 1;
 * if one is not, ok is 0 except with probability about 2^-127 over the seed (proof points in G1 / G2; on BLS12-381 the two sums are multiplied by
 * the G1 cofactor and the other factors raised to it). */
int zkmi_groth16_verify_aggregate(uint64_t vk_handle, const uint8_t* proofs_xyz, const uint8_t* publics, uint32_t n_signals, size_t n, const uint8_t seed[32], int8_t* codes,
                                  int* ok);
/* Multi-GPU proof (BASELINE configs[2]: MSMs sharded across the GPUs of a node). Every rank loads the shard of the
 * key that holds the witness-side bases of the variables [var_lo, var_hi) (sections 5-8) and the H bases [h_lo, h_hi) (section 9);
 * the section pointers of `zkey` are those of the FULL sections, the library slices them. zkmi_groth16_sums_dev runs the device
 * part of a proof on the FULL witness (buildABC, NTT chain, joinABC are replicated: they need no exchange) and returns this
 * shard's five partial MSM sums  jA | jB1 | jB2 | jC | jH  (Jacobian, 3*n8q bytes each, jB2 6*n8q: 7*3*n8q bytes in total).
 * The caller adds the sums of all ranks (one all-gather of < 1 KB per rank + zkmi_point_add) and zkmi_groth16_finish applies the
 * blinding and toAffine (:103-132, host, O(1)). With the full key, sums + finish == zkmi_groth16_prove_dev. */
int zkmi_groth16_load_shard(const zkmi_groth16_zkey* zkey, uint64_t zkey_cache_key, uint32_t var_lo, uint32_t var_hi, uint32_t h_lo, uint32_t h_hi);
int zkmi_groth16_sums_dev(uint64_t zkey_cache_key, const void* d_witness, uint8_t* sums);
/* Chain-parallel multi-GPU proof: the three iNTT -> coset -> NTT chains of src/groth16_prove.js:64-76 are independent until joinABC
 * (:79), so each runs on a different rank. zkmi_groth16_chains_dev runs buildABC (cheap, every owning rank) and the chains selected by
 * chain_mask (bit 0: A, 1: B, 2: C) on the full domain and writes their outputs (domain x 32 B, Montgomery) to d_a / d_b / d_c
 * (NULL for unselected chains). The owner of a chain sends rank j the slice [h_lo_j, h_hi_j) of its output (point-to-point over
 * xGMI, domain*32 bytes leave each owner in total); rank j joins its three slices (zkmi_groth16_join_abc_dev) into ITS H-MSM scalars and
 * zkmi_groth16_sums_h_dev runs the five MSMs of its key shard with them — no rank repeats another rank's transforms. */
int zkmi_groth16_chains_dev(uint64_t zkey_cache_key, const void* d_witness, unsigned chain_mask, void* d_a, void* d_b, void* d_c);
/* The shard's MSMs in two halves, so that no rank idles while transforms run elsewhere and slices travel: zkmi_groth16_sums_w_dev enqueues
 * the witness-side half (digit sorts of the witness, bucket accumulations B2, B1, A, C, the G2 bucket reduction — they need the witness
 * only) and returns at once; zkmi_groth16_sums_h_dev then enqueues the H half (digit sort of d_h_scalars, accumulation H, the batched G1
 * bucket reductions), waits and returns the sums. Without a preceding _sums_w_dev, _sums_h_dev runs both halves (r02 behaviour). */
int zkmi_groth16_sums_w_dev(uint64_t zkey_cache_key, const void* d_witness);
int zkmi_groth16_sums_h_dev(uint64_t zkey_cache_key, const void* d_witness, const void* d_h_scalars, uint8_t* sums);
int zkmi_groth16_finish(uint64_t zkey_cache_key, const uint8_t* sums, const uint8_t* r_mont, const uint8_t* s_mont, uint8_t* pi_a, uint8_t* pi_b, uint8_t* pi_c);

/* ---- PLONK prover: the per-element loops of src/plonk_prove.js and src/polynomial/polynomial.js as device kernels ---------
 * (SURVEY.md 8a rows a10-a12). All buffers are DEVICE pointers to Montgomery Fr elements; 32-byte constants are host
 * pointers (Montgomery). Polynomial lengths are in elements. */
/* Fr.w[i] (min.js:1@185893), needs no device */
int zkmi_fr_root(int curve, unsigned i, uint8_t* out32);
/* computeWirePolynomials gather (plonk_prove.js:267-283): A/B/C[i] = getWitness(map[i]) for i < n_constraints, 0 up to domain.
 * d_witness: n_witness elements (normal form, witness[0] already zeroed, :94-96); d_internal: the n_additions internal
 * signals (:174-204); maps are u32 arrays. Output is in the witness's (normal) form: run batchToMontgomery next (:285-287). */
int zkmi_plonk_gather_wires_dev(int curve, const void* d_witness, uint32_t n_witness, const void* d_internal, uint32_t n_additions,
                                const void* d_map_a, const void* d_map_b, const void* d_map_c, uint32_t n_constraints, uint32_t domain,
                                void* d_a, void* d_b, void* d_c);
/* the same with Fr.batchToMontgomery (:278) applied in the same pass: A/B/C come out in Montgomery form */
int zkmi_plonk_gather_wires_mont_dev(int curve, const void* d_witness, uint32_t n_witness, const void* d_internal, uint32_t n_additions,
                                     const void* d_map_a, const void* d_map_b, const void* d_map_c, uint32_t n_constraints, uint32_t domain,
                                     void* d_a, void* d_b, void* d_c);
/* calculateAdditions (src/plonk_prove.js:174-204, src/fflonk_prove.js:269-300): the internal signals of a PLONK / FFLONK key,
 *   internal[i] = factor1_i * getWitness(id1_i) + factor2_i * getWitness(id2_i),   getWitness as in :207-215 (n_vars = n_witness + n_additions),
 * computed on the device in ONE launch although an addition may read internal signals created before it (a dependency DAG of any depth; time grows
 * with the depth — a few microseconds per level — which is ceil(log2 k) for a k-term combination in keys written by plonk.setup, src/plonk_setup.js:176-212). d_additions: the zkey's additions section as it lies in the file (n_additions records of 72 bytes: u32 id1, u32 id2, factor1,
 * factor2 in Montgomery form). d_witness as for zkmi_plonk_gather_wires_dev. d_internal: n_additions elements, normal form (the
 * reference's buffInternalWitness). Stream-ordered: returns once enqueued. */
int zkmi_plonk_additions_dev(int curve, const void* d_additions, uint32_t n_additions, const void* d_witness, uint32_t n_witness, void* d_internal);
/* computeZ (plonk_prove.js:361-455): grand-product evaluations Z[0..domain) from the wire buffers (Montgomery) and the 4n
 * sigma evaluations (sampled at stride 4). Fails with "Copy constraints does not match" if Z[0] != 1. w_n = Fr.w[power]. */
int zkmi_plonk_compute_z_dev(int curve, const void* d_a, const void* d_b, const void* d_c, const void* d_s1e, const void* d_s2e,
                             const void* d_s3e, uint32_t domain, const uint8_t* beta, const uint8_t* gamma, const uint8_t* k1,
                             const uint8_t* k2, const uint8_t* w_n, void* d_z);
/* The same without the wait and without the Z[0] check: the caller compares Z[0] with one at its next synchronisation point and raises the
 * reference's "Copy constraints does not match" there (two proofs in flight from one host thread: the host must not block per kernel). */
int zkmi_plonk_compute_z_enqueue(int curve, const void* d_a, const void* d_b, const void* d_c, const void* d_s1e, const void* d_s2e,
                                 const void* d_s3e, uint32_t domain, const uint8_t* beta, const uint8_t* gamma, const uint8_t* k1,
                                 const uint8_t* k2, const uint8_t* w_n, void* d_z);
/* computeT (plonk_prove.js:516-628 with MulZ.mul2/mul4, mul_z.js:49-148): T and Tz over the 4n extended evaluation points.
 * lagrange = zkey section 13 on the device (per public input: n coefficients then 4n evaluations); pub_a = buffers.A. */
typedef struct zkmi_plonk_evals {
    const void *a, *b, *c, *z, *qm, *ql, *qr, *qo, *qc, *s1, *s2, *s3;     /* 4n evaluations each */
    const void* lagrange;
    const void* pub_a;
} zkmi_plonk_evals;
int zkmi_plonk_compute_t_dev(int curve, const zkmi_plonk_evals* ev, uint32_t domain, uint32_t n_public, const uint8_t* blind11 /* b1..b11 */,
                             const uint8_t* beta, const uint8_t* gamma, const uint8_t* alpha, const uint8_t* k1, const uint8_t* k2,
                             const uint8_t* w_n, const uint8_t* w_4n, const uint8_t* w_2, void* d_t, void* d_tz);
/* FFLONK quotient numerators (src/fflonk_prove.js): T0 (:415-504) over 4n points from a,b,c,ql,qr,qm,qo,qc,lagrange,pub_a of
 * `ev`; T1 / T1z (:667-718) over 2n points from the 4n evaluations of z and the Lagrange section (b789 = b7,b8,b9; w_2n =
 * Fr.w[power+1]); T2 / T2z (:720-815) over 4n points from a,b,c,z,s1,s2,s3 of `ev`. */
int zkmi_fflonk_t0_dev(int curve, const zkmi_plonk_evals* ev, uint32_t domain, uint32_t n_public, void* d_t0);
int zkmi_fflonk_t1_dev(int curve, const void* d_z4, const void* d_lagrange, uint32_t domain, const uint8_t* b789, const uint8_t* w_2n,
                       void* d_t1, void* d_t1z);
int zkmi_fflonk_t2_dev(int curve, const zkmi_plonk_evals* ev, uint32_t domain, const uint8_t* b789, const uint8_t* beta, const uint8_t* gamma,
                       const uint8_t* k1, const uint8_t* k2, const uint8_t* w_n, const uint8_t* w_4n, void* d_t2, void* d_t2z);
/* Polynomial.degree (polynomial.js:163-172): highest index of a non-zero coefficient, 0 if none */
int zkmi_poly_degree_dev(int curve, const void* d_p, size_t n, size_t* degree);
/* Keccak-256 with the original 0x01 padding (@noble/hashes keccak_256 as used by src/Keccak256Transcript.js:18-62); host only,
 * needs no device: the Fiat-Shamir transcript of the PLONK / FFLONK provers */
int zkmi_keccak256(const uint8_t* data, size_t len, uint8_t* out32);
/* Polynomial.add / sub with optional blinding value (polynomial.js:218-276): y[i] = y[i] +/- k*x[i], i < nx (k NULL = 1) */
int zkmi_poly_axpy_dev(int curve, void* d_y, const void* d_x, size_t nx, const uint8_t* k, int subtract);
/* Polynomial.mulScalar (:278-284) */
int zkmi_poly_scale_dev(int curve, void* d_p, size_t n, const uint8_t* k);
/* blindCoefficients (polynomial.js:68-93) on a buffer of n + count elements whose tail is zero: p[n+i] += f_i, p[i] -= f_i.
 * factors: count x 32 bytes (host, Montgomery), count <= 8. No host synchronisation. Per-call constants of every function of this section (factors, k, x, beta) travel as
 * kernel arguments: none of them costs an upload of its own. */
int zkmi_poly_blind_dev(int curve, void* d_p, size_t n, const uint8_t* factors, int count);
/* the same IN PLACE on a buffer with room for n + count elements of which only the first n were written: p[n+i] = f_i, p[i] -= f_i */
int zkmi_poly_blind_tail_dev(int curve, void* d_p, size_t n, const uint8_t* factors, int count);
/* A chain of Polynomial.add / sub / mulScalar / addScalar (polynomial.js:218-290) as ONE pass: out[i] = sum_j k_j p_j[i] (i < len_j) + (i == 0 ? constant : 0), i < out_len.
 * has_k = 0: k_j = 1 (pass -k for a subtraction), constant NULL = none, count <= 16, every len_j <= out_len; out may be one of the operands. Exact field arithmetic: the result is
 * the one the reference's sequence of calls leaves, whatever their order (src/plonk_prove.js:769-866 builds R and Wxi with 18 such calls). A term is 56 bytes without host
 * pointers, so that a binding can fill an array of them in one flat buffer (device pointer and length as 64-bit little-endian integers). */
typedef struct zkmi_poly_term { const void* d_p; uint64_t len; uint8_t k[32]; uint32_t has_k; uint32_t reserved; } zkmi_poly_term;
int zkmi_poly_lincomb_dev(int curve, void* d_out, size_t out_len, const zkmi_poly_term* terms, int count, const uint8_t* constant);
/* addScalar (polynomial.js:286-290): p[0] += value. No host synchronisation. */
int zkmi_poly_add_scalar_dev(int curve, void* d_p, const uint8_t* value);
/* Polynomial.evaluate (Horner, :174-184) as a parallel reduction; out = 32 bytes (host) */
int zkmi_poly_evaluate_dev(int curve, const void* d_p, size_t n, const uint8_t* x, uint8_t* out);
/* count <= 8 evaluations with ONE wait: polynomial q (lens[q] coefficients) at xs[32 q .. 32 q + 32) -> out[32 q ..] (round 4 of PLONK: six evaluations at two points,
 * src/plonk_prove.js:686-708). The power table of a point is built on the device; points that repeat share it. */
int zkmi_poly_evaluate_multi_dev(int curve, const void* const* d_polys, const size_t* lens, const uint8_t* xs, int count, uint8_t* out);
/* *all_zero = 1 iff p[0..n) are all zero (degree checks, plonk_prove.js:298-306, :645-647) */
int zkmi_poly_is_zero_dev(int curve, const void* d_p, size_t n, int* all_zero);
/* Polynomial.divZh(domainSize, extensions) (:592-615), in place; "Polynomial is not divisible" on a non-zero tail */
int zkmi_poly_div_zh_dev(int curve, void* d_p, size_t len, uint32_t domain, uint32_t extensions);
/* Polynomial.divByZerofier(n, beta) (:617-674): division by X^n - beta, in place (PLONK openings use n = 1, FFLONK n > 1) */
int zkmi_poly_div_by_zerofier_dev(int curve, void* d_p, size_t len, uint32_t n, const uint8_t* beta);
/* the same, enqueued only (no wait, no error from the division itself): the reference's divisibility test is "the n highest coefficients of the quotient are zero"
 * (:665-669) — the caller makes it at its next synchronisation point with zkmi_poly_is_zero_dev(p + len - n, n) and raises "Polynomial is not divisible" itself. */
int zkmi_poly_div_by_zerofier_enqueue(int curve, void* d_p, size_t len, uint32_t n, const uint8_t* beta);
/* Round 3 of PLONK (src/plonk_prove.js:649-672): T (t_len >= 3*domain + 6 coefficients, fewer read as zero) split into T1 = T[0, n) + b10 X^n (n + 1 coefficients),
 * T2 = T[n, 2n) - b10 + b11 X^n (n + 1), T3 = T[2n, 3n + 6) - b11 (n + 6): one launch instead of three zero fills, three copies and five single-coefficient reads / writes */
int zkmi_plonk_split_t_dev(int curve, const void* d_t, size_t t_len, uint32_t domain, const uint8_t* b10, const uint8_t* b11, void* d_t1, void* d_t2, void* d_t3);
/* CPolynomial.getPolynomial (src/polynomial/cpolynomial.js:53-73): out[i*n + j] = P_j[i] for i < lens[j] (d_polys[j] may be
 * NULL), zero elsewhere; n <= 16 component polynomials; out_len elements are written. */
int zkmi_cpoly_interleave_dev(int curve, const void* const* d_polys, const size_t* lens, int n, void* d_out, size_t out_len);

/* ---- group-element FFTs and G.batchApplyKey (ceremony side) -------------------------------------------------
 * curve.G1/G2.fft / .ifft (engine_fft for groups, min.js:1@215859: the Fr butterflies with "multiply by a twiddle" = G.timesFr) and, through
 * it, G.lagrangeEvaluations for 2^k <= 2^Fr.s points (src/powersoftau_preparephase2.js:87). n = 2^log_n affine points in (2*group*n8q bytes
 * each, Montgomery, all-zero = infinity), n affine points out, natural order; the inverse includes the factor 1/n. */
int zkmi_group_fft(int curve, int group, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, unsigned log_n, int inverse);
int zkmi_group_fft_dev(int curve, int group, const void* d_in, void* d_out, unsigned log_n, int inverse);
/* curve.G1/G2.batchApplyKey(buff, first, inc) (engine_applykey, min.js:1@211529; src/mpc_applykey.js:44-70): out_i = (first * inc^i) * P_i,
 * affine in and out; first / inc are Montgomery Fr elements (host pointers). */
int zkmi_group_batch_apply_key(int curve, int group, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, size_t n,
                               const uint8_t* first, const uint8_t* inc);
int zkmi_group_batch_apply_key_dev(int curve, int group, const void* d_in, void* d_out, size_t n, const uint8_t* first, const uint8_t* inc);
/* out_i = k * P_i for ONE scalar k (a Montgomery Fr element, host pointer): what G.batchApplyKey(buff, k, 1) computes, the shape of phase 2 of a Groth16
 * ceremony (src/zkey_contribute.js:90-92: sections L and H times 1 / delta). Affine in and out as above; d_out == d_in is allowed. group == 1 runs a kernel
 * of its own (the scalar is recoded once on the host, every lane takes the same branches), group == 2 the general kernel with inc = 1.
 * Refused while a pipeline slot holds work in flight. */
int zkmi_group_scale(int curve, int group, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, size_t n, const uint8_t* k_mont);
int zkmi_group_scale_dev(int curve, int group, const void* d_in, void* d_out, size_t n, const uint8_t* k_mont);

/* ---- the host side of a Groth16 phase-2 contribution (src/zkey_contribute.js, src/zkey_beacon.js, src/keypair.js); none of it needs a device --------
 * zkmi_phase2_key_from_seed: rng = ChaCha(seed8) (ffjavascript's: eight 32-bit seed words); prv_key = Fr.fromRng(rng) (32 bytes: the integer drawn is the
 *   element's Montgomery form), g1_s = G1.toAffine(G1.fromRng(rng)), g1_sx = prv_key * g1_s (affine Montgomery, 2 n8q bytes each).
 * zkmi_phase2_hash_to_g2: hashToG2(transcript) of src/keypair.js:24-36 for a 64-byte transcript hash, as an affine point (4 n8q bytes).
 * zkmi_point_mul: out = k * P for one affine point (2 * group * n8q bytes, all-zero = infinity) and a Montgomery Fr element k, affine out. */
int zkmi_phase2_key_from_seed(int curve, const uint32_t* seed8, uint8_t* prv_key, uint8_t* g1_s, uint8_t* g1_sx);
int zkmi_phase2_hash_to_g2(int curve, const uint8_t* transcript64, uint8_t* g2_sp);
int zkmi_point_mul(int curve, int group, const uint8_t* affine, const uint8_t* k_mont, uint8_t* out_affine);

/* ---- the H basis change of a Bellman-format phase-2 round trip (src/zkey_export_bellman.js:43-52, src/zkey_import_bellman.js:133-142) --
 * G1 only; n = 2^log_n = the key's domainSize, w = Fr.w[log_n + 1]. One upload, log_n + 3 or + 4 launches over one work array, one download.
 *   direction 0 (export): `in` holds n affine LEM points (section 9 of the key, all-zero = infinity); out = n - 1 points in the reference's uncompressed
 *     big-endian form (toRprUncompressed / batchLEMtoU, all-zero = infinity): point i = (-2 w^i) * G1.fft(in)_i. Index n - 1 is not computed.
 *   direction 1 (import): `in` holds n - 1 uncompressed points; out = n affine LEM points = G1.ifft([(-(1/2) w^-j) * P_j ..., infinity]), the 1 / n of the
 *     inverse transform folded into the one scalar of each point.
 * Export followed by import is not the identity: the coefficient export drops comes back as zero. The output pages' lengths add up to exactly the points
 * written. ZKMI_ERR_UNSUPPORTED for log_n < 1, log_n + 1 > Fr.s (28 on BN254, 32 on BLS12-381) and log_n > 28; ZKMI_ERR_INVALID for an unknown curve or
 * direction, a null pointer, page totals that do not match, or a pipeline slot with work in flight. The _dev twin runs on resident buffers (16-byte
 * aligned; d_in and d_out distinct). */
int zkmi_bellman_h_section(int curve, zkmi_pages in, unsigned log_n, int direction, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages);
int zkmi_bellman_h_section_dev(int curve, const void* d_in, void* d_out, unsigned log_n, int direction);

/* ---- verification of a Groth16 phase-2 key (src/zkey_verify_frominit.js, src/zkey_verify_fromr1cs.js) --------------------------------
 * The reference's generator by position. ChaCha(seed8) is ffjavascript's: the keystream in nextU32 order is word j = word j % 16 of block j / 16.
 * zkmi_chacha_words_dev: d_out[j] = keystream word first_word + j for j < n_words (32-bit words; first_word need not be a multiple of 16).
 * zkmi_chacha_fr_dev: the first n results of Fr.fromRng on a fresh ChaCha(seed8), as the raw 32-byte little-endian integers the reference keeps (the integer
 *   drawn IS the Montgomery form). Attempt k of the generator is words 8k .. 8k + 7 (limb i = w[2i] << 32 | w[2i + 1]), masked to the bit length of r and
 *   kept iff below r; output i is the i-th kept attempt. *words_consumed (may be NULL) = the position a sequential generator would be at after the n-th
 *   draw. A pure function of (curve, seed8, n); d_out (device memory, n x 32 bytes) must be 16-byte aligned. */
int zkmi_chacha_words_dev(const uint32_t seed8[8], uint64_t first_word, void* d_out, size_t n_words);
int zkmi_chacha_fr_dev(int curve, const uint32_t seed8[8], void* d_out, size_t n, uint64_t* words_consumed);
/* misc.sameRatio (src/misc.js:129-137) for n quadruples in one launch, one lane each: verdicts[i] = 1 iff e(g1s_i, g2sx_i) * e(-g1sx_i, g2s_i) == 1.
 * Points are affine Montgomery bytes as they lie in a zkey (2 n8q per G1 point, 4 n8q per G2 point; host pointers). A quadruple with any of its four
 * points at infinity (all-zero bytes) is 0 and pairs nothing, as in the reference. */
int zkmi_same_ratio_batch(int curve, const uint8_t* g1s, const uint8_t* g1sx, const uint8_t* g2s, const uint8_t* g2sx, size_t n, int8_t* verdicts);
/* The two sums of sectionHasSameRatio (src/zkey_verify_frominit.js:234-269) over two G1 sections of n affine points: out_a = sum s_i A_i,
 * out_b = sum s_i B_i with s_i = keystream word i of ChaCha(seed8) as a 4-byte scalar; the scalars are made on the device once and serve both sums.
 * The sums add, so the reference's chunks of 2^20 points are not observable. n == 0: both results are infinity (all-zero) and nothing else is done.
 * The two sums of sameRatioH (:271-350) for domainSize = 2^power. Fr(x): x taken as a Montgomery element.
 *   raw[0 .. domain - 2] = zkmi_chacha_fr_dev(seed8), raw[domain - 1] = 0
 *   out_r1 = sum fromMontgomery(raw_i) * (tau[domain + i] - tau[i]); the last term has scalar zero and tau[2 domain - 1] is never read, so tau_g1
 *            holds 2 domain - 1 points (all a ptau of the key's own power has)
 *   out_r2 = sum t_i H_i over the domain points of section 9, t = fromMontgomery(fft(applyKey(raw, -2, Fr.w[power + 1])))
 * power >= Fr.s (the reference's other branch: 2^28 on BN254) is refused with ZKMI_ERR_UNSUPPORTED.
 * Results are Jacobian, 3 n8q bytes, as zkmi_msm_dev writes them. Both calls are refused while a pipeline slot holds work in flight. */
int zkmi_phase2_section_ratio(int curve, zkmi_pages a, zkmi_pages b, size_t n, const uint32_t seed8[8], uint8_t* out_a, uint8_t* out_b);
int zkmi_phase2_h_ratio(int curve, zkmi_pages tau_g1, zkmi_pages h, uint32_t power, const uint32_t seed8[8], uint8_t* out_r1, uint8_t* out_r2);

/* ---- verification of a powers-of-tau file (src/powersoftau_verify.js) ---------------------------------------------------------------
 * zkmi_ptau_section_check: everything powersOfTau.verify needs of one section, from one upload. `tau` holds n_tau affine LEM points of `group` (section
 * 2, 3, 4 or 5); `lagrange` (NULL: the file has none) holds the 2^(top + 1) - 1 points of section 12, 13, 14 or 15, top = power + 1 for tauG1 and power
 * otherwise; zero_last is 1 for tauG1 alone, whose section holds 2^top - 1 points.
 *   u_out    the n_tau points in U form (zkmi_group_convert_dev), the bytes the reference hashes, into the caller's pages
 *   r1, r2   processSection (:340-396): r1 = sum_{i < n_tau - 1} s_i P_i, r2 = sum_{i < n_tau - 1} s_i P_{i+1}, s_i = keystream word i of
 *            ChaCha(pair_seed8) as a 4-byte scalar. The sums add, so the reference's chunks of 2^16 points and its extra scalar for the pair that
 *            straddles two chunks are this same formula. n_tau <= 1: both are infinity (all-zero).
 *   ladder   verifyLagrangeEvaluations (:398-491), only with `lagrange`: ladder[p] for p = 0 .. top is 1 iff
 *            sum_{i < 2^p} w_i tau_i == sum_{i < 2^p} fft_p(w)_i L_{2^p - 1 + i}, w_i = keystream word i of ChaCha(ladder_seed8), the generator restarted
 *            for every p. For p == top with zero_last, w_{2^p - 1} = 0 and tau_{2^p - 1} is never read. The left sides are running sums over the dyadic
 *            segments [2^(p-1), 2^p) with 4-byte scalars, so the tau section is walked once; the right sides transform the words widened to 32-byte
 *            normal-form elements (a transform is linear: the reference's batchToMontgomery / batchFromMontgomery pair drops out).
 * top > Fr.s is refused with ZKMI_ERR_UNSUPPORTED (BN254: a power-28 tauG1 section). r1, r2 are Jacobian, 3 * group * n8q bytes. Refused while a pipeline
 * slot holds work in flight.
 * zkmi_blake2b512_resume: misc.fromPartialHash(partial216) (src/misc.js:89-127: the 128-byte block buffer, the eight 64-bit state words as pairs of 32-bit
 * words, length - position in words 16 / 17, the position in the buffer in words 18 / 19), then .update(data).digest(). Host only, needs no device. */
int zkmi_ptau_section_check(int curve, int group, zkmi_pages tau, size_t n_tau, const zkmi_pages* lagrange, uint32_t top, int zero_last,
                            const uint32_t pair_seed8[8], const uint32_t ladder_seed8[8], uint8_t* const* u_out_ptr, const size_t* u_out_len,
                            int n_u_pages, uint8_t* r1, uint8_t* r2, int8_t* ladder);
int zkmi_blake2b512_resume(const uint8_t* partial216, const uint8_t* data, size_t len, uint8_t* out64);
/* keypair.createPTauKey (src/keypair.js:61-74) up to its G2 halves, for a beacon contribution: rng = ChaCha(seed8); three Fr.fromRng (tau, alpha, beta:
 * prv_keys, 3 x 32 bytes), then per key g1_s = G1.fromRng(rng) and g1_sx = prvKey * g1_s (3 x 2 n8q bytes each, affine Montgomery). Host only. */
int zkmi_ptau_key_from_seed(int curve, const uint32_t seed8[8], uint8_t* prv_keys, uint8_t* g1_s, uint8_t* g1_sx);

/* ---- the Lagrange sections of a prepared powers-of-tau file (src/powersoftau_preparephase2.js, src/powersoftau_convert.js) -----------
 * zkmi_ptau_lagrange_section: for p = first .. top, G.ifft of the first 2^p points of `tau` (affine LEM points of `group`: section 2, 3, 4 or 5), the
 * blocks back to back in the caller's pages: 2^(top + 1) - 2^first points, what the reference writes into section 12, 13, 14 or 15 power by power. With
 * zero_last (tauG1: top = power + 1) the last point of the top block is taken as infinity and never read, and the section holds 2^top - 1 points.
 * n_tau must equal 2^top - (zero_last ? 1 : 0); first <= top; first = top is the single transform powersOfTau.convert appends. All blocks are transformed
 * in one pass of top + 2 launches over one work array (csrc/ptau_lagrange.cuh). top > Fr.s and top > 28 are refused with ZKMI_ERR_UNSUPPORTED before
 * anything is allocated; refused while a pipeline slot holds work in flight. _dev: d_tau and d_out are device pointers of n_tau and
 * 2^(top + 1) - 2^first points; the result is complete once the library stream has drained (any later library call that reads d_out is ordered behind it). */
int zkmi_ptau_lagrange_section(int curve, int group, zkmi_pages tau, size_t n_tau, uint32_t first, uint32_t top, int zero_last, uint8_t* const* out_ptr,
                               const size_t* out_len, int n_out_pages);
int zkmi_ptau_lagrange_dev(int curve, int group, const void* d_tau, size_t n_tau, void* d_out, uint32_t first, uint32_t top, int zero_last);

/* ---- a phase-1 contribution (src/powersoftau_contribute.js, src/powersoftau_beacon.js) -------------------------------------------------
 * zkmi_ptau_contribute_section: everything a contribution needs of one section (2, 3, 4 or 5), from one upload. `in` holds n affine LEM points of `group`;
 * first / inc are Montgomery Fr elements (host pointers).
 *   lem   out_i = (first * inc^i) * P_i, what G.batchApplyKey(buff, first, inc) returns chunk after chunk: the bytes of the new file
 *   c     the same points in C form (G.batchLEMtoC: half the size), the bytes the response hash takes
 *   u     the same points in U form (G.batchLEMtoU), the bytes the next challenge hash takes
 * Each output is a list of pages whose lengths add up to exactly n points. group == 1 runs the per-lane-scalar kernel of csrc/ptau_contribute.cuh in slices
 * of at most 2^20 points (slice s starts from first * inc^(s * slice)), group == 2 the general kernel of zkmi_group_batch_apply_key_dev; both conversions run
 * on the resident LEM result. n == 0 returns ZKMI_OK and touches nothing. ZKMI_ERR_INVALID for an unknown curve or group, a null pointer, page totals that do
 * not match n, and while a pipeline slot holds work in flight (the slot keeps its work).
 * zkmi_blake2b512_partial: misc.toPartialHash (src/misc.js:111-127) of a fresh Blake2b-512 hasher after one `update` per chunk, the 216 bytes
 * zkmi_blake2b512_resume takes. The first 128 bytes are the reference's block buffer as those update calls leave it: a full block that more bytes of the
 * same call follow is hashed straight from the input and never copied, so the bytes beyond the position depend on how the data was cut into calls. Host only. */
int zkmi_ptau_contribute_section(int curve, int group, zkmi_pages in, size_t n, const uint8_t* first, const uint8_t* inc, uint8_t* const* lem_ptr, const size_t* lem_len,
                                 int n_lem_pages, uint8_t* const* c_ptr, const size_t* c_len, int n_c_pages, uint8_t* const* u_ptr, const size_t* u_len, int n_u_pages);
int zkmi_blake2b512_partial(const uint8_t* const* chunks, const size_t* lens, int n, uint8_t* partial216);

/* ---- the challenge / response round trip of phase 1 (src/powersoftau_challenge_contribute.js with applyKeyToChallengeSection of src/mpc_applykey.js,
 * src/powersoftau_import.js) ------------------------------------------------------------------------------------------------------------------
 * zkmi_ptau_challenge_section: one section of a response from one upload and one download. `in_u` holds n affine points of `group` in U form (a challenge
 * file's bytes); first / inc are Montgomery Fr elements (host pointers). On the device: batchUtoLEM, out_i = (first * inc^i) * P_i, then batchLEMtoC
 * (form == 0: half the size, what challengeContribute writes) or batchLEMtoU (form == 1, the reference's other branch). The multiplication runs in the slices
 * of zkmi_ptau_contribute_section (zkmi_diag_set_ptau_slice applies), group 1 on its kernel, group 2 on the per-lane-scalar kernel of csrc/ptau_challenge.cuh.
 * The points need not lie in the r-torsion; coordinates that are not on the curve give unspecified points.
 * zkmi_ptau_import_section: one section of an import from one upload and two downloads. `in_c` holds n points in C form (a response file's bytes); on the
 * device batchCtoLEM (the new file's bytes) and, on the resident result, batchLEMtoU (the bytes the next challenge hash takes). ZKMI_ERR_INVALID when some
 * x has no point on the curve, as in zkmi_group_convert.
 * Both: each output is a list of pages whose lengths add up to exactly n points. n == 0 returns ZKMI_OK and touches nothing. ZKMI_ERR_INVALID for an unknown
 * curve, group or form, a null pointer, page totals that do not match n, and while a pipeline slot holds work in flight (the slot keeps its work);
 * ZKMI_ERR_UNSUPPORTED for n >= 2^31. */
int zkmi_ptau_challenge_section(int curve, int group, zkmi_pages in_u, size_t n, const uint8_t* first, const uint8_t* inc, uint8_t* const* out_ptr, const size_t* out_len,
                                int n_out_pages, int form);
int zkmi_ptau_import_section(int curve, int group, zkmi_pages in_c, size_t n, uint8_t* const* lem_ptr, const size_t* lem_len, int n_lem_pages, uint8_t* const* u_ptr,
                             const size_t* u_len, int n_u_pages);

/* curve.G1/G2.batchLEMtoU / batchUtoLEM / batchLEMtoC / batchCtoLEM (engine_batchconvert over wasmcurves' g1m_/g2m_batch*, min.js:1@128060;
 * callers src/powersoftau_import.js:159,221, src/powersoftau_contribute.js:145,176, src/powersoftau_export_challenge.js:72,
 * src/powersoftau_verify.js:358, src/mpc_applykey.js:64-70, src/zkey_export_bellman.js:36-83, src/zkey_new.js:103-115,373).
 *   LEM = affine little-endian Montgomery (2*group*n8q bytes, all-zero = infinity), U = affine big-endian normal form (same size, Fq2 as
 *   c1 || c0, all-zero = infinity), C = x alone big-endian (group*n8q bytes; first byte |= 0x80 when y > (p-1)/2, 0x40 = infinity).
 * n points in, n points out. C_TO_LEM recovers y by a square root and returns ZKMI_ERR_INVALID when some x has no point on the curve. */
#define ZKMI_CONV_LEM_TO_U 0
#define ZKMI_CONV_U_TO_LEM 1
#define ZKMI_CONV_LEM_TO_C 2
#define ZKMI_CONV_C_TO_LEM 3
int zkmi_group_convert(int curve, int group, int kind, zkmi_pages in, uint8_t* const* out_ptr, const size_t* out_len, int n_out_pages, size_t n);
int zkmi_group_convert_dev(int curve, int group, int kind, const void* d_in, void* d_out, size_t n);

/* ---- witness check: wtns.check (src/wtns_check.js) ------------------------------------------------------------------------------------
 * Constraint i holds iff evalA * evalB == evalC in Fr; an evaluation is the sum of coef * w[signal] over the DISTINCT signals of the combination, with
 * the LAST coefficient the file gives for a signal. Coefficients and witness values are any 256-bit little-endian value, taken mod r; w[0] need not be 1;
 * a zero coefficient and an empty combination are legal.
 *   zkmi_r1cs_load     `constraints` = r1cs section 2 as it lies in the file (per constraint three combinations, each u32 n then n x (u32 signal, 32-byte
 *                      coefficient)); bytes after the last constraint are ignored. The term counts are read on the host, the section goes up once and the
 *                      resident layout is built on the device (csrc/r1cs_check.cuh). ZKMI_ERR_INVALID: an unknown curve, a null pointer, cache_key 0, a
 *                      section that ends inside a constraint, a signal id >= n_vars, another r1cs resident under the key (the same one: ZKMI_OK, nothing is
 *                      done). ZKMI_ERR_UNSUPPORTED: 3 * n_constraints >= 2^31, 2^32 terms or more. n_constraints == 0 loads.
 *   zkmi_r1cs_check    n_witnesses witnesses of n_vars x 32 bytes each, one after the other in host memory (wtns section 2); witness_len must be
 *                      n_witnesses * n_vars * 32. first_bad[k] = index of the first constraint witness k fails, 0xFFFFFFFF when it satisfies all (with
 *                      n_constraints == 0: always). A large batch is cut into passes that fit the work memory. ZKMI_ERR_INVALID: cache_key 0, no r1cs
 *                      resident under the key, a null pointer, a wrong witness_len; the resident r1cs is left as it was.
 *   zkmi_r1cs_check_dev the same for witnesses already in device memory (a resident prover gating on the verdict); first_bad is host memory.
 *   zkmi_r1cs_release  frees the layout and its work memory (an unknown key: ZKMI_OK).
 * All of them use the active pipeline slot's stream and compute no MSM: not refused while a slot holds work in flight. Complete on return. */
int zkmi_r1cs_load(int curve, zkmi_pages constraints, uint32_t n_constraints, uint32_t n_vars, uint64_t cache_key);
int zkmi_r1cs_check(uint64_t cache_key, const uint8_t* witnesses, size_t witness_len, uint32_t n_witnesses, uint32_t* first_bad);
int zkmi_r1cs_check_dev(uint64_t cache_key, const void* d_witnesses, size_t witness_len, uint32_t n_witnesses, uint32_t* first_bad);
int zkmi_r1cs_release(uint64_t cache_key);


/* ---- utilities --------------------------------------------------------------------------------------------------- */
/* Page-lock caller-owned host memory for device transfers (hipHostRegister): shared-memory regions through which the processes of a
 * multi-GPU proof exchange chain outputs (js/groth16_shards.js). Optional: transfers from unregistered memory work, slower. */
int zkmi_host_register(void* host_ptr, size_t bytes);
int zkmi_host_unregister(void* host_ptr);
/* ---- GPU-to-GPU exchange between the processes of a multi-GPU proof (snarkjs_amd/csrc/peer.hip) --------------------------------------
 * The reference spreads one multiExp / one proof over its workers by handing them chunk buffers and folding the results on the host
 * (ffjavascript engine_multiexp, min.js:1@214651; worker dispatch @207729). Here a worker is a process that owns one GPU; the bulk data of a
 * sharded Groth16 proof (the three chain outputs, domain x 32 bytes each) moves device to device: the owner of a chain exports the buffer
 * that holds its output, every other process opens the handle once and pulls ITS slice per proof — over xGMI between two GPUs, inside HBM
 * when two processes share a device. Control (who is ready, the 7 x 3 x n8q-byte partial sums) stays on the host's own channel.
 *   zkmi_ipc_export: handle (ZKMI_IPC_HANDLE_BYTES, plain bytes: send them over any channel) for a device pointer of this process
 *                    (zkmi_dev_alloc or any hipMalloc'ed range; interior pointers allowed).
 *   zkmi_ipc_open:   device pointer in THIS process for a handle (peer access is enabled on first use); *bytes_visible (optional) = bytes
 *                    from the pointer to the end of the exported allocation. A handle exported by the calling process resolves to the
 *                    original pointer. zkmi_ipc_close drops the mapping (the exporter keeps the memory).
 *   zkmi_peer_copy:  d_dst <- d_src for `bytes` bytes, complete on return. The copies run on a stream of their own, NOT behind what the library
 *                    stream has queued (a shard process has its witness-side accumulations there when the slices arrive).
 *                    zkmi_peer_copy_async: queued only; zkmi_peer_fence() makes the library stream wait (an event, no host wait) for every
 *                    copy queued so far, so that the next call (zkmi_groth16_join_abc_dev) sees the data. The exporter must have finished
 *                    writing (its zkmi_groth16_chains_dev returned) before a peer reads, and must not overwrite the buffer until every peer
 *                    has finished its copy: the host orders this (js/groth16_shards.js: a chain is announced when complete; the next proof
 *                    starts only after every worker has delivered its sums). */
#define ZKMI_IPC_HANDLE_BYTES 96
int zkmi_ipc_export(const void* d_ptr, uint8_t* handle);
int zkmi_ipc_open(const uint8_t* handle, void** d_ptr, size_t* bytes_visible);
int zkmi_ipc_close(void* d_ptr);
int zkmi_peer_copy(void* d_dst, const void* d_src, size_t bytes);
int zkmi_peer_copy_async(void* d_dst, const void* d_src, size_t bytes);
int zkmi_peer_fence(void);
/* Curve of a resident Groth16 key (ZKMI_CURVE_*), -1 when the key is not loaded: bindings size their output buffers from the KEY, not from
 * a caller-supplied curve id. */
int zkmi_groth16_key_curve(uint64_t key);
/* Error recovery for the split proof (zkmi_groth16_sums_w_dev / _sums_h_dev, _submit / _collect): waits for the device, then forgets any
 * half-enqueued or in-flight proof of this key in both pipeline slots, so that the next proof starts clean after a failed exchange. */
int zkmi_groth16_reset(uint64_t key);
/* G.toAffine on host for one Jacobian point (tiny; used by bindings to normalise results). */
int zkmi_to_affine(int curve, int group, const uint8_t* jacobian, uint8_t* affine);
/* G.add on host for two Jacobian points (O(1)): folds the per-GPU partial results of a sharded MSM
 * (reference: host-side `G.add` over chunk results, min.js:1@214651). Needs no device. */
int zkmi_point_add(int curve, int group, const uint8_t* a_jacobian, const uint8_t* b_jacobian, uint8_t* out_jacobian);

#ifdef __cplusplus
}
#endif
#endif /* ZKMI_H */

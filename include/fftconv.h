/*
 * fftconv.h -- C ABI of the MI355X-native partitioned FFT convolver.
 *
 * Drop-in boundary for Sin-tel/fft-convolution's `Convolution` trait
 * (src/lib.rs:5-14):
 *
 *     trait Convolution: Clone {
 *         fn init(response: &[f32], max_block_size: usize, max_response_length: usize) -> Self;
 *         fn update(&mut self, response: &[f32]);          // real-time safe
 *         fn reset(&mut self);
 *         fn process(&mut self, input: &[f32], output: &mut [f32]);
 *     }
 *
 * Every handle is a *batch* of `channels` independent convolvers that share
 * one geometry (block size, max response length) and live on one GPU.  A
 * handle created by the single-channel `*_init` entry point is a batch of 1
 * and is the exact counterpart of one reference instance.  Batched host
 * buffers are laid out channel-major: sample j of channel c at [c*len + j]
 * (or [c*stride + j] where a stride is taken).
 *
 * Errors: where the reference panics (assert!/panic!/todo!/slice bounds) the
 * call returns a negative status and leaves the instance unchanged; the
 * message is available from fftconv_last_error().  A runtime FFT error
 * (realfft's C2R rejecting a non-finite DC/Nyquist bin) zero-fills that
 * channel's output and leaves its block state where the reference leaves it
 * (src/fft_convolver.rs:264-267); it is not an error status.
 *
 * There is no CPU fallback: creating a handle without a usable gfx950 device
 * fails with FFTCONV_E_DEVICE.
 *
 * Streams: every `void *hip_stream` argument is a hipStream_t, and NULL is
 * HIP's null (legacy default) stream -- the same meaning it has in every HIP
 * API and the stream PyTorch's default stream maps to.  A call enqueued on a
 * stream is ordered after the handle's previous work wherever that ran (one
 * event wait when the stream differs from the last one used), and anything
 * enqueued on the same stream afterwards sees its results.  Host-synchronous
 * entry points use the handle's own (non-blocking) stream and wait for it;
 * *_synchronize waits for all of a handle's work.
 */
#ifndef FFTCONV_H
#define FFTCONV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFTCONV_ABI_VERSION 1

enum {
    FFTCONV_OK = 0,
    FFTCONV_E_INVALID = -1,       /* a reference panic!/assert!/slice-bounds precondition */
    FFTCONV_E_UNIMPLEMENTED = -2, /* a reference todo!() */
    FFTCONV_E_UNSUPPORTED = -3,   /* geometry outside this build (block size > 2^22) */
    FFTCONV_E_DEVICE = -4,        /* HIP runtime error / no device */
    FFTCONV_E_NOMEM = -5
};

typedef struct fftconv_uniform fftconv_uniform;     /* FFTConvolver        src/fft_convolver.rs:86-307 */
typedef struct fftconv_twostage fftconv_twostage;   /* TwoStageFFTConvolver src/fft_convolver.rs:323-512 */
typedef struct fftconv_crossfade fftconv_crossfade; /* CrossfadeConvolver<FFTConvolver | TwoStageFFTConvolver> src/crossfade_convolver.rs:10-105 */
typedef struct fftconv_matrix fftconv_matrix;       /* inputs x outputs FFTConvolver instances, summed per output (below) */
typedef struct fftconv_matrix_sparse fftconv_matrix_sparse; /* one FFTConvolver instance per listed (output, input) pair (below) */
typedef struct fftconv_matrix_sparse_crossfade fftconv_matrix_sparse_crossfade; /* one CrossfadeConvolver per listed pair (below) */
typedef struct fftconv_matrix_lookahead fftconv_matrix_lookahead; /* the matrix with far-row windows (below) */
typedef struct fftconv_matrix_sparse_lookahead fftconv_matrix_sparse_lookahead; /* the sparse matrix with far-row windows (below) */
typedef struct fftconv_matrix_crossfade fftconv_matrix_crossfade; /* inputs x outputs CrossfadeConvolver<FFTConvolver> instances (below) */
typedef struct fftconv_matrix_lookahead_crossfade fftconv_matrix_lookahead_crossfade; /* the crossfaded matrix over two lookahead matrices (below) */
typedef struct fftconv_matrix_twostage fftconv_matrix_twostage;   /* inputs x outputs TwoStageFFTConvolver instances (below) */
typedef struct fftconv_matrix_sparse_twostage fftconv_matrix_sparse_twostage; /* one TwoStageFFTConvolver per listed pair (below) */

/* ---- library ----------------------------------------------------------- */
int fftconv_abi_version(void);
const char *fftconv_last_error(void);            /* thread-local, "" if none */
int fftconv_device_count(void);                   /* visible HIP devices, 0 if none */
size_t fftconv_complex_size(size_t size);         /* src/fft_convolver.rs:52-54 */
size_t fftconv_compute_tail_block_size(size_t head_len, size_t response_len); /* :520-526 */

/* ---- Fft (src/fft_convolver.rs:7-50) ----------------------------------- */
/* The reference's public real FFT (realfft's RealToComplex / ComplexToReal of
 * length n; Fft::init takes any usize, :30-34) as batched device transforms.
 * n: any length in 1..2^21, or a power of two up to 2^23.
 *   - A power of two runs the convolver's own kernels (n > 16384: the
 *     four-step passes of the long-block path), so a spectrum here is
 *     bit-identical to the convolver's.
 *   - Any other length runs Bluestein's chirp-z transform over power-of-two
 *     FFTs of P >= 2n-1 points (its tables are cached per length, at most
 *     256 MiB of device memory, least recently used first out).  Those
 *     spectra are within f32 rounding of an f64 DFT, not bit-identical to any
 *     convolver kernel (the convolver's block sizes are powers of two).
 * A row of bins is 2*(n/2+1) floats: n+2 for even n, n+1 for odd n.
 * Forward (Fft::forward :36-39): rows of n reals -> n/2+1 bins,
 * interleaved (re, im), unnormalised, DC (and, for even n, Nyquist)
 * imaginary parts 0.
 * Inverse (Fft::inverse :41-49): n/2+1 bins -> n reals divided by n;
 * d_status[row] (optional) = 1 where realfft returns FftError::InputValues
 * (non-zero DC imaginary part, or for even n a non-zero Nyquist imaginary
 * part; the transform runs with those parts as 0).  Such a row is NOT divided
 * by n: Fft::inverse returns the error through `?` (:42) before its
 * normalisation loop (:44-46).  Strides in floats; enqueued on `hip_stream`
 * (NULL = HIP's null stream). */
int fftconv_fft_forward(int device, size_t n, size_t rows, const float *d_in, size_t in_stride, float *d_out,
                        size_t out_stride, void *hip_stream);
int fftconv_fft_inverse(int device, size_t n, size_t rows, const float *d_in, size_t in_stride, float *d_out,
                        size_t out_stride, int *d_status, void *hip_stream);
/* Host-memory forms, rows packed ([rows][n] reals, [rows][2*(n/2+1)] bin floats);
 * synchronous (temporary device buffers: not for the real-time path). */
int fftconv_fft_forward_host(int device, size_t n, size_t rows, const float *input, float *output);
int fftconv_fft_inverse_host(int device, size_t n, size_t rows, const float *input, float *output, int *status);
/* Tuning knob (process-wide): spectral-MAC scan variant of the fused kernel,
 * -1 = automatic (default: nontemporal loads when the per-step H+X stream
 * exceeds the Infinity Cache, plain loads otherwise -- the load policy never
 * changes a result bit; the pipelined full-block step when B <= 512 and a
 * channel's FDL holds <= 16384 bins, chosen per geometry, never by channel
 * count, so channel shards stay bit-identical; for a CrossfadeConvolver
 * with a longer FDL, one workgroup runs A and B on one FDL stream, which
 * never changes a result bit),
 * else bit 0 = zig-zag segment order on alternate blocks, bit 1 =
 * nontemporal H/X loads, bit 2 = no pipelined step (every call computes
 * its pre_multiplied at block start, as the reference does) -- when none
 * of bits 0-2 is set, the automatic load and step policy stays --, bit 3 = no
 * crossfade pair launch (A and B stream the shared FDL separately), bit 4 =
 * no lookahead step (see below), bit 5 = lookahead launches without anchors
 * (every full block sums all its FDL rows itself; bit-identical to the
 * lookahead path, for tests), bit 6 = crossfade on the lookahead step with
 * the stand-alone mix kernel (by default B's launch mixes in its epilogue,
 * from gains A's launch precomputed; bit-identical either way), bit 7 = IR
 * transforms (init / update) one segment per workgroup (by default one per
 * wave for 64 <= B <= 1024; bit-identical), bit 8 = two-stage tail0 runs
 * per head block (by default its blocks are convolved together at the end
 * of each tail period; read when a TwoStageFFTConvolver is created), bit 9 =
 * that end-of-period flush in five kernels instead of the one fused kernel
 * that is the default (head block 64; bit-identical), bit 10 = no far-row windows for B >= 1024 (every
 * one-block call sums its far rows itself; bit-identical), bit 11 =
 * process_device_steps launches once per call (by default, for 64 <= B <= 512,
 * a TwoStageFFTConvolver's aligned calls inside one tail period, and the
 * calls of an FFTConvolver batch on the generic / pipelined step with at most
 * two channels per CU, run as ONE launch in which each channel's workgroup
 * loops over its calls; bit-identical).
 * The table above the VARIANT_ enum in fft-convolution_amd/csrc/variant.hpp
 * has one row per bit, and says which are read per launch and which when a
 * handle is created.
 * Lookahead (automatic for standalone FFTConvolver batches with
 * 128 <= B <= 512 and >= 40 segments, full-block calls from an empty input
 * buffer): the FDL sum of each block is re-associated in time over a near
 * level and three anchor levels with geometric periods -- the step sums
 * rows 1..4 itself, an anchor every 4 blocks sums rows 5..16 for the next 4
 * blocks, one every 16 blocks rows 17..64 for the next 16, one every 64
 * blocks rows >= 65 for the next 64 -- so a full-block call streams ~1/10
 * of the reference's bytes; its summation order does not depend on the
 * channel index, the shard or the call history (bit-identical to summing
 * every row).
 * -1 selects automatic; any other negative value is FFTCONV_E_INVALID.
 * Results agree within f32 rounding across variants. */
int fftconv_set_kernel_variant(int variant);
int fftconv_get_kernel_variant(void);
/* Tuning knob (process-wide): FDL rows the pipelined step leaves to its
 * stream waves while its first wave runs the transform chain; -1 = automatic
 * (all of them: the first wave never streams).  Does not change results beyond
 * f32 summation order. */
int fftconv_set_pipeline_lag(int rows);
int fftconv_get_pipeline_lag(void);
/* Pinned host staging of update() (process-wide, read when a handle is
 * created).  A standalone FFTConvolver batch, and a crossfade, reserve
 * channels x max_response_length floats of pinned host memory at init, so
 * update() copies the response and returns without waiting for the upload
 * (src/lib.rs:8 asks update to be real-time safe: it never allocates).  A cap
 * in bytes (0 = none, the default) -- or a reservation the host refuses, which
 * falls back to smaller ones down to one response row -- makes update() stream
 * the rows through the stage in chunks, waiting for each chunk's copy before
 * refilling it: no allocation either way, same results. */
int fftconv_set_host_stage_limit(size_t bytes);
size_t fftconv_get_host_stage_limit(void);

/* ---- FFTConvolver (uniformly partitioned, zero latency) ---------------- */
/* FFTConvolver::init, src/fft_convolver.rs:105-172.  NULL on error. */
fftconv_uniform *fftconv_uniform_init(const float *response, size_t response_len,
                                      size_t max_block_size, size_t max_response_length);
/* Batched init on `device`: channel c's response is responses[c*response_stride ..
 * + response_len] (host memory). */
fftconv_uniform *fftconv_uniform_init_batch(int device, size_t channels, const float *responses,
                                            size_t response_len, size_t response_stride,
                                            size_t max_block_size, size_t max_response_length);
/* FFTConvolver::update, src/fft_convolver.rs:174-213; every channel gets the
 * same response.  No allocation (staging is reserved at init). */
int fftconv_uniform_update(fftconv_uniform *h, const float *response, size_t response_len);
/* Per-channel responses, host memory, channel c at responses[c*stride ..]. */
int fftconv_uniform_update_batch(fftconv_uniform *h, const float *responses, size_t response_len,
                                 size_t response_stride);
/* One channel only. */
int fftconv_uniform_update_channel(fftconv_uniform *h, size_t channel, const float *response,
                                   size_t response_len);
/* update() from device-resident responses (channel c at d_responses[c*stride],
 * stride 0 = one response for every channel), enqueued on `hip_stream`
 * (NULL = HIP's null stream) without a host synchronisation or an allocation. */
int fftconv_uniform_update_device(fftconv_uniform *h, const float *d_responses, size_t response_len,
                                  size_t response_stride, void *hip_stream);
/* FFTConvolver::reset, src/fft_convolver.rs:296-306 (all channels). */
int fftconv_uniform_reset(fftconv_uniform *h);
/* FFTConvolver::process, src/fft_convolver.rs:215-295, host buffers:
 * input [channels][input_len], output [channels][output_len]; reads
 * input[0..output_len] of each channel (input_len >= output_len, else
 * FFTCONV_E_INVALID like the reference's slice panic).  Synchronous. */
int fftconv_uniform_process(fftconv_uniform *h, const float *input, size_t input_len,
                            float *output, size_t output_len);
/* Same on device-resident buffers, enqueued on `hip_stream` (NULL = HIP's
 * null stream), asynchronous: channel c reads d_input[c*in_stride ..
 * + len] and writes d_output[c*out_stride .. + len]. */
int fftconv_uniform_process_device(fftconv_uniform *h, const float *d_input, size_t in_stride,
                                   float *d_output, size_t out_stride, size_t len, void *hip_stream);
/* `steps` consecutive process() calls of `len` samples each, from one host
 * call: call k reads d_input + k*in_step (channel stride in_stride) and writes
 * d_output + k*out_step.  Identical to `steps` calls of _process_device; it
 * removes the per-call host overhead when blocks are already resident.
 *
 * A standalone batch on the lookahead step (128 <= B <= 512, 40 or more
 * segments) called with len == block size runs a call of 16 or more steps as
 * a batch: four launches per chunk of up to 64 steps instead of one per step,
 * each IR row and delay-line row read once per chunk (bit-identical; cfg2:
 * 11.4 us per step in 32-step calls against 16.6).  The batch takes the
 * handle's partial-sum windows, so the next _process_device call (or a steps
 * call shorter than 16) re-enters with a full sum of every channel, ~400 us
 * at cfg2, and until it has, steps calls of any length take the batch.  A
 * caller that alternates steps calls and single _process_device calls pays
 * that entry at every switch (612 us per pair of one call and one 16-step
 * call, measured): it should submit everything through one of the two, or
 * set kernel-variant bit 11 (2048), which keeps _process_device_steps on one
 * launch per step. */
int fftconv_uniform_process_device_steps(fftconv_uniform *h, const float *d_input, size_t in_stride,
                                         size_t in_step, float *d_output, size_t out_stride,
                                         size_t out_step, size_t len, size_t steps, void *hip_stream);
/* #[derive(Clone)]: a deep, device-side copy of every buffer and scalar. */
fftconv_uniform *fftconv_uniform_clone(const fftconv_uniform *h);
void fftconv_uniform_destroy(fftconv_uniform *h);
int fftconv_uniform_synchronize(fftconv_uniform *h);
size_t fftconv_uniform_channels(const fftconv_uniform *h);
/* anchor workgroups per channel of the lookahead step, 0 = not used */
int fftconv_uniform_lookahead_parts(const fftconv_uniform *h);
/* window rows per channel of the generic step's far-row windows (automatic
 * for standalone batches with B >= 1024 and >= 24 segments: an
 * anchor every P blocks sums rows >= P for a channel's next P one-block
 * calls; bit-identical to summing them every block), 0 = not used */
int fftconv_uniform_far_windows(const fftconv_uniform *h);
/* (tests) with FFTCONV_LA_PROBE=1 in the environment when the handle was
 * created, the lookahead launches make their anchors wait for the steps and
 * read the live state words, which they do not compute from (they use the
 * launch-start copies, la.hpp la_anchor_state): the number of live words
 * found already rewritten by the same launch so far; -1 when the probe is
 * off (the default) */
int fftconv_uniform_lookahead_probe(const fftconv_uniform *h);
size_t fftconv_uniform_block_size(const fftconv_uniform *h);   /* next_power_of_two(max_block_size) */
size_t fftconv_uniform_seg_count(const fftconv_uniform *h);
/* segments_ir[segment] of one channel (src/fft_convolver.rs:92): B+1 bins,
 * interleaved (re, im), into host `out` ((B+1)*2 floats) */
int fftconv_uniform_ir_spectrum(const fftconv_uniform *h, size_t channel, size_t segment, float *out);
/* copies {current, active_seg_count, input_buffer_fill} of one channel */
int fftconv_uniform_channel_state(const fftconv_uniform *h, size_t channel, size_t out3[3]);

/* ---- TwoStageFFTConvolver (head block + García-optimal tail block) ----- */
fftconv_twostage *fftconv_twostage_init(const float *response, size_t response_len,
                                        size_t max_block_size, size_t max_response_length);
fftconv_twostage *fftconv_twostage_init_batch(int device, size_t channels, const float *responses,
                                              size_t response_len, size_t response_stride,
                                              size_t max_block_size, size_t max_response_length);
/* todo!() in the reference (src/fft_convolver.rs:408-410): FFTCONV_E_UNIMPLEMENTED. */
int fftconv_twostage_update(fftconv_twostage *h, const float *response, size_t response_len);
int fftconv_twostage_reset(fftconv_twostage *h);
/* len must be <= max_block_size (assert at src/fft_convolver.rs:414); input and
 * output both [channels][len]. */
int fftconv_twostage_process(fftconv_twostage *h, const float *input, float *output, size_t len);
int fftconv_twostage_process_device(fftconv_twostage *h, const float *d_input, size_t in_stride,
                                    float *d_output, size_t out_stride, size_t len, void *hip_stream);
int fftconv_twostage_process_device_steps(fftconv_twostage *h, const float *d_input, size_t in_stride,
                                          size_t in_step, float *d_output, size_t out_stride,
                                          size_t out_step, size_t len, size_t steps, void *hip_stream);
fftconv_twostage *fftconv_twostage_clone(const fftconv_twostage *h);
void fftconv_twostage_destroy(fftconv_twostage *h);
int fftconv_twostage_synchronize(fftconv_twostage *h);
size_t fftconv_twostage_tail_block_size(const fftconv_twostage *h);

/* ---- CrossfadeConvolver<FFTConvolver> ---------------------------------- */
/* Convolution::init, src/crossfade_convolver.rs:46-49: crossfade_samples =
 * response_len, hold = min(max_block_size, response_len). */
fftconv_crossfade *fftconv_crossfade_init(const float *response, size_t response_len,
                                          size_t max_block_size, size_t max_response_length);
fftconv_crossfade *fftconv_crossfade_init_batch(int device, size_t channels, const float *responses,
                                                size_t response_len, size_t response_stride,
                                                size_t max_block_size, size_t max_response_length);
/* CrossfadeConvolver::new, src/crossfade_convolver.rs:19-43.  `convolver` is
 * cloned (the reference moves it; the caller keeps ownership of its handle). */
fftconv_crossfade *fftconv_crossfade_new(const fftconv_uniform *convolver, size_t max_response_length,
                                         size_t max_buffer_size, size_t crossfade_samples);
/* CrossfadeConvolver<TwoStageFFTConvolver> (the reference's CrossfadeConvolver
 * is generic over `Convolution`, src/crossfade_convolver.rs:11,45-49): the same
 * handle type and the same functions below.  Its update() reaches
 * TwoStageFFTConvolver::update, todo!() (src/fft_convolver.rs:408-410), before
 * anything changes: FFTCONV_E_UNIMPLEMENTED and the handle is unchanged.
 * process() needs input_len == max_buffer_size <= the inner head block size
 * (:412-414 and the head / tail slice bounds). */
fftconv_crossfade *fftconv_crossfade_init_twostage(const float *response, size_t response_len,
                                                   size_t max_block_size, size_t max_response_length);
fftconv_crossfade *fftconv_crossfade_init_twostage_batch(int device, size_t channels, const float *responses,
                                                         size_t response_len, size_t response_stride,
                                                         size_t max_block_size, size_t max_response_length);
fftconv_crossfade *fftconv_crossfade_new_twostage(const fftconv_twostage *convolver, size_t max_response_length,
                                                  size_t max_buffer_size, size_t crossfade_samples);
/* src/crossfade_convolver.rs:51-64; same response for every channel. */
int fftconv_crossfade_update(fftconv_crossfade *h, const float *response, size_t response_len);
int fftconv_crossfade_update_batch(fftconv_crossfade *h, const float *responses, size_t response_len,
                                   size_t response_stride);
/* update() from device-resident responses, stream-ordered (see uniform). */
int fftconv_crossfade_update_device(fftconv_crossfade *h, const float *d_responses, size_t response_len,
                                    size_t response_stride, void *hip_stream);
/* todo!() in the reference (src/crossfade_convolver.rs:80-82): FFTCONV_E_UNIMPLEMENTED. */
int fftconv_crossfade_reset(fftconv_crossfade *h);
/* src/crossfade_convolver.rs:66-78: input_len >= max_buffer_size and
 * output_len <= max_buffer_size (the reference's slice bounds). */
int fftconv_crossfade_process(fftconv_crossfade *h, const float *input, size_t input_len,
                              float *output, size_t output_len);
int fftconv_crossfade_process_device(fftconv_crossfade *h, const float *d_input, size_t in_stride,
                                     float *d_output, size_t out_stride, size_t output_len,
                                     void *hip_stream);
int fftconv_crossfade_process_device_steps(fftconv_crossfade *h, const float *d_input, size_t in_stride,
                                           size_t in_step, float *d_output, size_t out_stride,
                                           size_t out_step, size_t output_len, size_t steps,
                                           void *hip_stream);
int fftconv_crossfade_is_crossfading(const fftconv_crossfade *h); /* :85-92, 1/0 */
fftconv_crossfade *fftconv_crossfade_clone(const fftconv_crossfade *h);
void fftconv_crossfade_destroy(fftconv_crossfade *h);
int fftconv_crossfade_synchronize(fftconv_crossfade *h);

/* ---- MatrixConvolver: multi-input multi-output partitioned convolution ----
 *     y[o] = sum_i x[i] * h[o][i]        (o < outputs, i < inputs)
 * A matrix (inputs I, outputs O, block B, max_response_length) behaves as I*O
 * FFTConvolver instances (o, i) (src/fft_convolver.rs:86-307), all created,
 * updated and reset together with the same response_len: instance (o, i)
 * processes input i, output o is the sum over i of the outputs of (o, i).  The
 * state machine of :215-295 runs in lockstep, so one {current,
 * active_seg_count, input_buffer_fill} describes the matrix (fftconv_matrix_state).
 * The device keeps one frequency-domain delay line per input, sums the spectra
 * per output and runs one inverse transform per output: results equal the
 * summed instances within f32 rounding, not bitwise.  Outputs do not depend on
 * `outputs`: a matrix split by outputs over several handles (or GPUs) computes
 * bit-identical rows.
 * Two departures from the per-instance reference:
 *  - Non-finite samples are outside the parity contract.  The per-instance
 *    "C2R error -> zero-fill, state frozen" path (:264-267) cannot be
 *    reproduced with a shared delay line: output values are unspecified while
 *    a non-finite sample is inside the delay line or the overlap, the state
 *    advances normally, and outputs are exact again once the sample has left.
 *  - Updates are updates of the whole matrix: update() zeroes overlap and
 *    pre_multiplied per instance (:186-188), which the matrix keeps summed per
 *    output, so updating one instance alone cannot match the definition.
 *    fftconv_matrix_update_pairs (and the crossfaded matrix's, below) is
 *    therefore DEFINED as update(R'), R' = the response set the matrix holds
 *    with the listed pairs replaced: every output's overlap and pre_multiplied
 *    are zeroed as update does, and only the listed pairs are uploaded and
 *    transformed.  The sparse matrix and the sparse crossfade have
 *    update_pairs over their listed pairs; the lookahead and two-stage
 *    matrices offer the whole update only.
 * Responses: pair p = o * inputs + i at responses + p * response_stride
 * (response_stride 0 = one response for every pair).  Supported blocks:
 * 32 <= next_power_of_two(max_block_size) <= 8192, else FFTCONV_E_UNSUPPORTED;
 * inputs == 0, outputs == 0 or response_len > max_response_length is
 * FFTCONV_E_INVALID; init returns NULL on error (fftconv_last_error). */
fftconv_matrix *fftconv_matrix_init(int device, size_t inputs, size_t outputs, const float *responses,
                                    size_t response_len, size_t response_stride, size_t max_block_size,
                                    size_t max_response_length);
/* :174-213 for every pair; asynchronous like fftconv_uniform_update. */
int fftconv_matrix_update(fftconv_matrix *h, const float *responses, size_t response_len,
                          size_t response_stride);
int fftconv_matrix_update_device(fftconv_matrix *h, const float *d_responses, size_t response_len,
                                 size_t response_stride, void *hip_stream);
/* update(R'), bit for bit in outputs and state: R' = the responses of the last
 * init / update with the n_pairs listed pairs replaced, at THAT call's
 * response_len (row n of `responses`, response_len samples, belongs to pair
 * (pair_out[n], pair_in[n]) and is zero-padded to it; a longer response_len is
 * FFTCONV_E_INVALID).  The pair list is strictly ascending in o * inputs + i,
 * as fftconv_matrix_sparse_init's: an unsorted, repeated or out-of-range pair is
 * FFTCONV_E_INVALID and the handle is unchanged; an empty list is update(R).
 * response_stride 0 = one response for every listed pair.  pair_out / pair_in
 * are host arrays in both variants.  No allocation; the host waits no more
 * than in fftconv_matrix_update. */
int fftconv_matrix_update_pairs(fftconv_matrix *h, size_t n_pairs, const uint32_t *pair_out,
                                const uint32_t *pair_in, const float *responses, size_t response_len,
                                size_t response_stride);
int fftconv_matrix_update_pairs_device(fftconv_matrix *h, size_t n_pairs, const uint32_t *pair_out,
                                       const uint32_t *pair_in, const float *d_responses, size_t response_len,
                                       size_t response_stride, void *hip_stream);
int fftconv_matrix_reset(fftconv_matrix *h); /* :296-306 */
/* input [inputs][input_len], output [outputs][output_len], host memory;
 * input_len < output_len is FFTCONV_E_INVALID. */
int fftconv_matrix_process(fftconv_matrix *h, const float *input, size_t input_len, float *output,
                           size_t output_len);
/* device memory, stream-ordered: input i at d_input + i * in_stride, output o
 * at d_output + o * out_stride (strides in floats). */
int fftconv_matrix_process_device(fftconv_matrix *h, const float *d_input, size_t in_stride, float *d_output,
                                  size_t out_stride, size_t len, void *hip_stream);
/* `steps` consecutive process_device calls, call k at d_input + k * in_step /
 * d_output + k * out_step; the same bits as the separate calls. */
int fftconv_matrix_process_device_steps(fftconv_matrix *h, const float *d_input, size_t in_stride,
                                        size_t in_step, float *d_output, size_t out_stride, size_t out_step,
                                        size_t len, size_t steps, void *hip_stream);
fftconv_matrix *fftconv_matrix_clone(const fftconv_matrix *h);
void fftconv_matrix_destroy(fftconv_matrix *h);
int fftconv_matrix_synchronize(fftconv_matrix *h);
size_t fftconv_matrix_inputs(const fftconv_matrix *h);
size_t fftconv_matrix_outputs(const fftconv_matrix *h);
size_t fftconv_matrix_block_size(const fftconv_matrix *h);
size_t fftconv_matrix_seg_count(const fftconv_matrix *h);
/* workgroups that share one output's spectral sum, for the current
 * active_seg_count: a function of (inputs, block, seg_count, active) only. */
int fftconv_matrix_mac_parts(const fftconv_matrix *h);
/* {current, active_seg_count, input_buffer_fill} as of the calls enqueued so far */
int fftconv_matrix_state(const fftconv_matrix *h, size_t out3[3]);

/* ---- SparseMatrixConvolver: matrix convolution over a listed pair set ----
 *     y[o] = sum over the listed pairs (o, i) of x[i] * h[(o, i)]
 * A sparse matrix has I inputs, O outputs and N >= 1 pairs (o_n, i_n), strictly
 * ascending in (o, i): sorted, no duplicates.  It behaves as N FFTConvolver
 * instances (src/fft_convolver.rs:86-307), one per listed pair, all created,
 * updated and reset together with the same response_len: instance n processes
 * input i_n, output o is the sum of the instances listed for it.  An output
 * with no listed pair is 0.0 for every sample of every call; an input that no
 * pair reads is accepted and ignored.  One {current, active_seg_count,
 * input_buffer_fill} describes the handle (fftconv_matrix_sparse_state).  The
 * pattern is fixed for the life of the handle; update replaces the N responses.
 * Only the listed pairs are stored, uploaded, transformed and streamed.
 * The dense matrix's two departures carry over unchanged: non-finite samples
 * are outside the parity contract, and only whole-matrix update is offered.
 * Responses: pair n, in list order, at responses + n * response_stride
 * (response_stride 0 = one response for every pair).
 * Order of summation (part of the contract), the dense matrix's with an
 * output's pair list in place of 0..I-1; k_o = the pairs of output o:
 *  - the rows of output o are H[pair e][s] (.) X[i_e][(current + s) % active],
 *    s >= 1, pair e = the e-th entry of output o's list and i_e its input,
 *    flattened pair-major in list order: r = e * (active - 1) + s - 1;
 *  - output o has P_o parts (fftconv_matrix_sparse_output_parts): the rule of
 *    fftconv_matrix_mac_parts with inputs := k_o, a function of output o's own
 *    list and active_seg_count only;
 *  - the split into parts and row groups, the order inside a group, of the
 *    groups and of the parts are the dense matrix's;
 *  - the finishing launch adds the row-0 terms X[i_e][current] (.) H[pair e][0]
 *    in ascending e.
 * So (1) output o is bit-identical to the single output of a dense
 * fftconv_matrix with k_o inputs that holds the responses h[pair e] and is fed
 * x[i_e] in list order, and (2) an output's bits depend on nothing outside its
 * own pair list and the inputs it names: a pattern split by outputs over
 * several handles (or GPUs) computes bit-identical rows.
 * Errors: pairs == 0, inputs == 0, outputs == 0, a pair index out of range, a
 * pair list that is not strictly ascending, or response_len >
 * max_response_length is FFTCONV_E_INVALID; a block outside 32..8192
 * (next_power_of_two(max_block_size)) or indices past 32 bits is
 * FFTCONV_E_UNSUPPORTED; init returns NULL on error (fftconv_last_error).
 * Crossfaded switching of a sparse matrix is fftconv_matrix_sparse_crossfade
 * (below); far-row windows for a sparse matrix with long responses and small
 * blocks are the fftconv_matrix_sparse_lookahead handle, below; two-stage
 * partitioning over a pattern is the fftconv_matrix_sparse_twostage handle
 * (below).  Out of scope: changing the pattern after init. */
fftconv_matrix_sparse *fftconv_matrix_sparse_init(int device, size_t inputs, size_t outputs, size_t pairs,
                                                  const uint32_t *pair_out, const uint32_t *pair_in,
                                                  const float *responses, size_t response_len,
                                                  size_t response_stride, size_t max_block_size,
                                                  size_t max_response_length);
/* :174-213 for every listed pair; asynchronous like fftconv_uniform_update: no
 * allocation, no host wait.  active_seg_count = ceil(response_len / block),
 * current is left alone (:186-190). */
int fftconv_matrix_sparse_update(fftconv_matrix_sparse *h, const float *responses, size_t response_len,
                                 size_t response_stride);
int fftconv_matrix_sparse_update_device(fftconv_matrix_sparse *h, const float *d_responses, size_t response_len,
                                        size_t response_stride, void *hip_stream);
/* update(R') at the response_len of the last init / update, defined as
 * fftconv_matrix_update_pairs is, with "pair" = a listed pair: the list is
 * (pair_out[n], pair_in[n]), strictly ascending in (o, i), and every entry must
 * belong to the pattern -- one that does not is FFTCONV_E_INVALID ("pair (o, i)
 * is not in the pattern"), the handle unchanged.  Only the listed pairs are
 * uploaded and transformed. */
int fftconv_matrix_sparse_update_pairs(fftconv_matrix_sparse *h, size_t n_pairs, const uint32_t *pair_out,
                                       const uint32_t *pair_in, const float *responses, size_t response_len,
                                       size_t response_stride);
int fftconv_matrix_sparse_update_pairs_device(fftconv_matrix_sparse *h, size_t n_pairs, const uint32_t *pair_out,
                                              const uint32_t *pair_in, const float *d_responses, size_t response_len,
                                              size_t response_stride, void *hip_stream);
int fftconv_matrix_sparse_reset(fftconv_matrix_sparse *h); /* :296-306 */
/* input [inputs][input_len], output [outputs][output_len], host memory;
 * input_len < output_len is FFTCONV_E_INVALID. */
int fftconv_matrix_sparse_process(fftconv_matrix_sparse *h, const float *input, size_t input_len, float *output,
                                  size_t output_len);
/* device memory, stream-ordered: input i at d_input + i * in_stride, output o
 * at d_output + o * out_stride (strides in floats). */
int fftconv_matrix_sparse_process_device(fftconv_matrix_sparse *h, const float *d_input, size_t in_stride,
                                         float *d_output, size_t out_stride, size_t len, void *hip_stream);
/* `steps` consecutive process_device calls, call k at d_input + k * in_step /
 * d_output + k * out_step; the same bits as the separate calls. */
int fftconv_matrix_sparse_process_device_steps(fftconv_matrix_sparse *h, const float *d_input, size_t in_stride,
                                               size_t in_step, float *d_output, size_t out_stride, size_t out_step,
                                               size_t len, size_t steps, void *hip_stream);
fftconv_matrix_sparse *fftconv_matrix_sparse_clone(const fftconv_matrix_sparse *h);
void fftconv_matrix_sparse_destroy(fftconv_matrix_sparse *h);
int fftconv_matrix_sparse_synchronize(fftconv_matrix_sparse *h);
size_t fftconv_matrix_sparse_inputs(const fftconv_matrix_sparse *h);
size_t fftconv_matrix_sparse_outputs(const fftconv_matrix_sparse *h);
size_t fftconv_matrix_sparse_pairs(const fftconv_matrix_sparse *h);
size_t fftconv_matrix_sparse_block_size(const fftconv_matrix_sparse *h);
size_t fftconv_matrix_sparse_seg_count(const fftconv_matrix_sparse *h);
/* P_o: the workgroups that share output `output`'s spectral sum, for the
 * current active_seg_count (1 for an output without pairs; 0 for a bad index) */
int fftconv_matrix_sparse_output_parts(const fftconv_matrix_sparse *h, size_t output);
/* {current, active_seg_count, input_buffer_fill} as of the calls enqueued so far */
int fftconv_matrix_sparse_state(const fftconv_matrix_sparse *h, size_t out3[3]);

/* ---- MatrixLookaheadConvolver: far-row windows for the matrix ----
 * Definition: exactly fftconv_matrix's -- I*O FFTConvolver instances (o, i) in
 * lockstep, output o the sum over i, one {current, active_seg_count,
 * input_buffer_fill} -- with the same two departures (non-finite samples are
 * outside the parity contract; only whole-matrix update).  What differs is the
 * schedule of the spectral sum, and with it the order of summation.
 * With the period Q = fftconv_matrix_lookahead_period() (8; part of the
 * contract) the rows H[o][i][s] (.) X[i][(current + s) % active] of an output
 * are split at Q.  Near rows 1 <= s < Q are summed on every block.  Far rows
 * Q <= s < active are summed by an anchor once every Q blocks: output o anchors
 * on the blocks t = o (mod Q), t = the handle's count of started blocks, and
 * one walk over its far rows produces the far sums ("window") of blocks t ..
 * t + Q - 1, so every far H row is read once per Q blocks.  After init, reset,
 * update and while current >= active (after a shrinking update) an output has
 * no window until its next anchor, at most Q - 1 blocks later; until then it
 * sums its far rows in full on every block.
 * Order of summation (part of the contract): pre[o] = near[o] + far[o], then
 * the row-0 terms X[i][current] (.) H[o][i][0] in ascending i.
 *  - near[o]: the rows (i, s), 1 <= s < min(Q, active), flattened i-major, in
 *    Pn parts (fftconv_matrix_lookahead_near_parts: the rule of
 *    fftconv_matrix_mac_parts on the near row count); inside a part the row
 *    groups and their order are the dense matrix's; parts added ascending.
 *  - far[o]: the rows (i, s), Q <= s < active, flattened i-major, in Pf parts
 *    (fftconv_matrix_lookahead_far_parts: the same rule on the far row count;
 *    0 when active <= Q, and then pre[o] = near[o]); inside a part each row
 *    group takes a contiguous, ascending sub-range of ceil(rows per part /
 *    groups) rows; groups added ascending, parts added ascending.
 * Both counts are functions of (inputs, active_seg_count, Q) only.  A block
 * served from a window and a block that sums everything itself perform the same
 * operations in the same order, so outputs do not depend on the anchor phase,
 * on fftconv_matrix_lookahead_set_windows, on `outputs` (a matrix split by
 * outputs over handles or GPUs computes bit-identical rows), or on how calls
 * are grouped (process_device_steps equals the separate calls).  They equal
 * fftconv_matrix's within f32 rounding, not bitwise.
 * Supported blocks: 32 <= next_power_of_two(max_block_size) <= 512, else
 * FFTCONV_E_UNSUPPORTED (use fftconv_matrix there); other errors as
 * fftconv_matrix_init.  Everything is reserved at init: update allocates
 * nothing and does not wait on the host.
 * The sparse matrix has the same windows as the fftconv_matrix_sparse_lookahead
 * handle, below; the crossfaded and two-stage matrices stay without lookahead. */
fftconv_matrix_lookahead *fftconv_matrix_lookahead_init(int device, size_t inputs, size_t outputs,
                                                        const float *responses, size_t response_len,
                                                        size_t response_stride, size_t max_block_size,
                                                        size_t max_response_length);
int fftconv_matrix_lookahead_update(fftconv_matrix_lookahead *h, const float *responses, size_t response_len,
                                    size_t response_stride);
int fftconv_matrix_lookahead_update_device(fftconv_matrix_lookahead *h, const float *d_responses,
                                           size_t response_len, size_t response_stride, void *hip_stream);
int fftconv_matrix_lookahead_reset(fftconv_matrix_lookahead *h); /* :296-306 */
int fftconv_matrix_lookahead_process(fftconv_matrix_lookahead *h, const float *input, size_t input_len,
                                     float *output, size_t output_len);
int fftconv_matrix_lookahead_process_device(fftconv_matrix_lookahead *h, const float *d_input, size_t in_stride,
                                            float *d_output, size_t out_stride, size_t len, void *hip_stream);
int fftconv_matrix_lookahead_process_device_steps(fftconv_matrix_lookahead *h, const float *d_input,
                                                  size_t in_stride, size_t in_step, float *d_output,
                                                  size_t out_stride, size_t out_step, size_t len, size_t steps,
                                                  void *hip_stream);
/* the clone carries the windows and the block count: it continues bit for bit */
fftconv_matrix_lookahead *fftconv_matrix_lookahead_clone(const fftconv_matrix_lookahead *h);
void fftconv_matrix_lookahead_destroy(fftconv_matrix_lookahead *h);
int fftconv_matrix_lookahead_synchronize(fftconv_matrix_lookahead *h);
size_t fftconv_matrix_lookahead_inputs(const fftconv_matrix_lookahead *h);
size_t fftconv_matrix_lookahead_outputs(const fftconv_matrix_lookahead *h);
size_t fftconv_matrix_lookahead_block_size(const fftconv_matrix_lookahead *h);
size_t fftconv_matrix_lookahead_seg_count(const fftconv_matrix_lookahead *h);
/* {current, active_seg_count, input_buffer_fill} as of the calls enqueued so far */
int fftconv_matrix_lookahead_state(const fftconv_matrix_lookahead *h, size_t out3[3]);
int fftconv_matrix_lookahead_period(void); /* Q */
int fftconv_matrix_lookahead_near_parts(const fftconv_matrix_lookahead *h);
int fftconv_matrix_lookahead_far_parts(const fftconv_matrix_lookahead *h);
/* on = 0: no output anchors, every block sums its far rows in full (the same
 * bits; for tests and measurements).  on = 1 (default): anchors resume at each
 * output's next slot. */
int fftconv_matrix_lookahead_set_windows(fftconv_matrix_lookahead *h, int on);
/* outputs that anchor when the next block starts (0 while windows are off,
 * active <= Q or current >= active) */
int fftconv_matrix_lookahead_anchors(const fftconv_matrix_lookahead *h);

/* ---- SparseMatrixLookaheadConvolver: far-row windows for the sparse matrix ----
 * Definition: exactly fftconv_matrix_sparse's -- I inputs, O outputs, N >= 1
 * pairs strictly ascending in (o, i), N FFTConvolver instances in lockstep, one
 * per listed pair; an output without pairs is 0.0, an input nobody reads is
 * accepted; one {current, active_seg_count, input_buffer_fill}; the pattern is
 * fixed for the life of the handle; the dense matrix's departures carry over.
 * What differs is the schedule of the spectral sum, which is
 * fftconv_matrix_lookahead's with the same period Q =
 * fftconv_matrix_lookahead_period(): output o anchors on the blocks t = o
 * (mod Q), one walk over its far rows produces the far sums of blocks t .. t +
 * Q - 1; after init, reset, update, update_pairs and while current >= active
 * an output sums its far rows in full until its next anchor.  update_pairs
 * drops the windows of every output, the untouched ones' too.
 * Order of summation (part of the contract): fftconv_matrix_lookahead's with
 * output o's pair list (k_o entries, entry e = the e-th pair listed for o, i_e
 * its input) in place of 0..I-1: pre[o] = near[o] + far[o], then the row-0
 * terms X[i_e][current] (.) H[pair e][0] in ascending e.
 *  - near[o]: the rows (e, s), 1 <= s < min(Q, active), flattened pair-major,
 *    in Pn_o parts (fftconv_matrix_sparse_lookahead_near_parts: the rule of
 *    fftconv_matrix_lookahead_near_parts on k_o * (min(Q, active) - 1) rows);
 *    groups and the order inside a part as fftconv_matrix_lookahead's near sum.
 *  - far[o]: the rows (e, s), Q <= s < active, flattened pair-major, in Pf_o
 *    parts (fftconv_matrix_sparse_lookahead_far_parts: the same rule on k_o *
 *    (active - Q) rows; 0 when active <= Q or k_o = 0, and then pre[o] =
 *    near[o]); contiguous rows per group, groups and parts added ascending, as
 *    fftconv_matrix_lookahead's far sum.
 * So (1) a block served from a window and a block that sums everything itself
 * perform the same operations in the same order: outputs do not depend on the
 * anchor phase, on fftconv_matrix_sparse_lookahead_set_windows, on how calls
 * are grouped, or on the load policy; (2) output o is bit-identical to the
 * single output of a dense fftconv_matrix_lookahead with k_o inputs that holds
 * the responses h[pair e] and is fed x[i_e] in list order; (3) an output's bits
 * depend on nothing outside its own pair list and the inputs it names: a
 * pattern split by outputs over several handles (or GPUs) computes
 * bit-identical rows.  Results equal fftconv_matrix_sparse's within f32
 * rounding, not bitwise.
 * Supported blocks: 32 <= next_power_of_two(max_block_size) <= 512, else
 * FFTCONV_E_UNSUPPORTED (use fftconv_matrix_sparse there); other errors as
 * fftconv_matrix_sparse_init.  Everything is reserved at init: update and
 * update_pairs allocate nothing and do not wait on the host.
 * Every function below is its fftconv_matrix_sparse_* / fftconv_matrix_lookahead_*
 * namesake. */
fftconv_matrix_sparse_lookahead *fftconv_matrix_sparse_lookahead_init(int device, size_t inputs, size_t outputs,
                                                                      size_t pairs, const uint32_t *pair_out,
                                                                      const uint32_t *pair_in, const float *responses,
                                                                      size_t response_len, size_t response_stride,
                                                                      size_t max_block_size,
                                                                      size_t max_response_length);
int fftconv_matrix_sparse_lookahead_update(fftconv_matrix_sparse_lookahead *h, const float *responses,
                                           size_t response_len, size_t response_stride);
int fftconv_matrix_sparse_lookahead_update_device(fftconv_matrix_sparse_lookahead *h, const float *d_responses,
                                                  size_t response_len, size_t response_stride, void *hip_stream);
int fftconv_matrix_sparse_lookahead_update_pairs(fftconv_matrix_sparse_lookahead *h, size_t n_pairs,
                                                 const uint32_t *pair_out, const uint32_t *pair_in,
                                                 const float *responses, size_t response_len, size_t response_stride);
int fftconv_matrix_sparse_lookahead_update_pairs_device(fftconv_matrix_sparse_lookahead *h, size_t n_pairs,
                                                        const uint32_t *pair_out, const uint32_t *pair_in,
                                                        const float *d_responses, size_t response_len,
                                                        size_t response_stride, void *hip_stream);
int fftconv_matrix_sparse_lookahead_reset(fftconv_matrix_sparse_lookahead *h); /* :296-306 */
int fftconv_matrix_sparse_lookahead_process(fftconv_matrix_sparse_lookahead *h, const float *input, size_t input_len,
                                            float *output, size_t output_len);
int fftconv_matrix_sparse_lookahead_process_device(fftconv_matrix_sparse_lookahead *h, const float *d_input,
                                                   size_t in_stride, float *d_output, size_t out_stride, size_t len,
                                                   void *hip_stream);
int fftconv_matrix_sparse_lookahead_process_device_steps(fftconv_matrix_sparse_lookahead *h, const float *d_input,
                                                         size_t in_stride, size_t in_step, float *d_output,
                                                         size_t out_stride, size_t out_step, size_t len, size_t steps,
                                                         void *hip_stream);
/* the clone carries the windows, the plan and the block count: it continues bit for bit */
fftconv_matrix_sparse_lookahead *fftconv_matrix_sparse_lookahead_clone(const fftconv_matrix_sparse_lookahead *h);
void fftconv_matrix_sparse_lookahead_destroy(fftconv_matrix_sparse_lookahead *h);
int fftconv_matrix_sparse_lookahead_synchronize(fftconv_matrix_sparse_lookahead *h);
size_t fftconv_matrix_sparse_lookahead_inputs(const fftconv_matrix_sparse_lookahead *h);
size_t fftconv_matrix_sparse_lookahead_outputs(const fftconv_matrix_sparse_lookahead *h);
size_t fftconv_matrix_sparse_lookahead_pairs(const fftconv_matrix_sparse_lookahead *h);
size_t fftconv_matrix_sparse_lookahead_block_size(const fftconv_matrix_sparse_lookahead *h);
size_t fftconv_matrix_sparse_lookahead_seg_count(const fftconv_matrix_sparse_lookahead *h);
/* {current, active_seg_count, input_buffer_fill} as of the calls enqueued so far */
int fftconv_matrix_sparse_lookahead_state(const fftconv_matrix_sparse_lookahead *h, size_t out3[3]);
/* Pn_o and Pf_o of output `output` for the current active_seg_count (0 for a bad index) */
int fftconv_matrix_sparse_lookahead_near_parts(const fftconv_matrix_sparse_lookahead *h, size_t output);
int fftconv_matrix_sparse_lookahead_far_parts(const fftconv_matrix_sparse_lookahead *h, size_t output);
/* on = 0: no output anchors, every block sums its far rows in full (the same bits) */
int fftconv_matrix_sparse_lookahead_set_windows(fftconv_matrix_sparse_lookahead *h, int on);
/* outputs with at least one pair that anchor when the next block starts (0
 * while windows are off, active <= Q or current >= active) */
int fftconv_matrix_sparse_lookahead_anchors(const fftconv_matrix_sparse_lookahead *h);

/* ---- MatrixCrossfadeConvolver: crossfaded response switching for the matrix ----
 * A matrix crossfade (inputs I, outputs O) behaves as I*O reference
 * CrossfadeConvolver<FFTConvolver> instances (o, i) (src/crossfade_convolver.rs:
 * 3-105), all created and updated together with the same lengths: instance
 * (o, i) processes input i, output o is the sum over i.  Every instance's
 * crossfader is in lockstep, so the handle has one Crossfader and one pending
 * response.  The device mixes the per-output sums, mix(sum_i a, sum_i b), not
 * the per-instance mixes: equal to the definition within f32 rounding, not
 * bitwise; in hold and Reached samples the mix returns a or b unchanged.
 * Mirrored from the reference:
 *  - new (:19-43): the convolver is cloned into A and B, hold =
 *    min(max_buffer_size, max_response_length), the stored response has
 *    max_response_length samples.  init (:46-49) = new(matrix init(...),
 *    response_len, max_block_size, response_len).
 *  - update (:51-64): not crossfading -> the idle convolver is updated and the
 *    fade starts at once; crossfading -> the response is stored (zero-padded)
 *    and applied by the first process() after the fade; response_len longer
 *    than the stored length is FFTCONV_E_INVALID, handle unchanged.  No
 *    allocation, no host wait.
 *  - process (:66-78): BOTH convolvers advance by max_buffer_size samples
 *    whatever output_len is; input_len < max_buffer_size or output_len >
 *    max_buffer_size is FFTCONV_E_INVALID.
 *  - reset is todo!() (:80-82): FFTCONV_E_UNIMPLEMENTED.
 * The matrix's departures carry over: non-finite samples are outside the
 * contract, and an update is an update of the whole matrix -- update_pairs
 * (below) is update(R') with the work of the listed pairs.  Pairs and strides as
 * fftconv_matrix_*.
 * Paths (fftconv_matrix_crossfade_path), chosen by the handle's state only --
 * every path computes the same bits:
 *   0  composition: A and B as two plain matrices, then the mix kernel.  Taken
 *      when A and B are not in step, or after set_fused(h, 0).
 *   1  fused, both convolvers live (a fade is under way): one forward
 *      transform per input for both delay lines, every delay-line row streamed
 *      once for both responses, the mix in the finish kernel's epilogue.
 *   2  fused, one convolver idle (no fade under way): the convolver that is not
 *      heard keeps only its delay line; its multiply-accumulate, inverse
 *      transform and overlap are skipped (exact: its next event is update(),
 *      which zeroes what was skipped, :186-188 of fft_convolver.rs).
 * A and B are in step while they have had equal {current, active_seg_count,
 * input_buffer_fill} and active_seg_count > 0 at every call since creation; an
 * update to another ceil(response_len / block) ends that for good.
 * Every supported block size (32..8192) runs fused: the finish kernel keeps
 * A's samples in the output buffer between its two passes and reads the fade
 * curve from a device table, so it needs no more LDS than the plain matrix. */
fftconv_matrix_crossfade *fftconv_matrix_crossfade_init(int device, size_t inputs, size_t outputs,
                                                        const float *responses, size_t response_len,
                                                        size_t response_stride, size_t max_block_size,
                                                        size_t max_response_length);
/* `convolver` is cloned (the caller keeps ownership of its handle). */
fftconv_matrix_crossfade *fftconv_matrix_crossfade_new(const fftconv_matrix *convolver, size_t max_response_length,
                                                       size_t max_buffer_size, size_t crossfade_samples);
int fftconv_matrix_crossfade_update(fftconv_matrix_crossfade *h, const float *responses, size_t response_len,
                                    size_t response_stride);
int fftconv_matrix_crossfade_update_device(fftconv_matrix_crossfade *h, const float *d_responses,
                                           size_t response_len, size_t response_stride, void *hip_stream);
/* update_pairs(pairs, responses, len) is update(R'), bit for bit in outputs and
 * in state (is_crossfading, path, what a later call does); R' = the base set
 * with the listed pairs replaced, at the base set's length len':
 *  - base set: the pending stored response if one is pending (len' = the
 *    stored length, max_response_length of new()), else the responses of the
 *    convolver the crossfader targets -- the one heard or faded into (len' =
 *    the response_len of that convolver's last init / update);
 *  - row n of `responses` (response_len samples) belongs to pair (pair_out[n],
 *    pair_in[n]) and is zero-padded to len'; response_len > len' is
 *    FFTCONV_E_INVALID; while a fade is under way response_len beyond the
 *    stored length is the reference's assert, as for update;
 *  - the pair list is strictly ascending in o * inputs + i: an unsorted,
 *    repeated or out-of-range pair is FFTCONV_E_INVALID, the handle unchanged;
 *    an empty list is update(base set);
 *  - so: no fade under way -> the swap happens at once; else the rows are
 *    stored and applied by the first process() after the fade; a second
 *    update_pairs during the fade merges into the first (the later call wins a
 *    pair listed twice); a later whole update replaces a pending partial one.
 * The work is proportional to what changed.  The handle keeps the set D of
 * pairs whose spectra may differ between its two convolvers (empty after new /
 * init, every pair after a whole update).  A partial swap copies the spectra of
 * D minus the listed pairs from the target convolver, transforms the listed
 * pairs, and leaves D = the listed pairs: one launch.  Where no spectra exist to
 * copy from -- a whole response is pending -- the stored rows are patched and
 * the whole swap runs (D = every pair).  The one unsupported case: a partial
 * update during a fade when ceil(stored length / block) differs from the
 * target convolver's active_seg_count (zero-padding cannot reproduce update
 * then): FFTCONV_E_UNSUPPORTED, handle unchanged.
 * pair_out / pair_in are host arrays in both variants; response_stride 0 = one
 * response for every listed pair.  No allocation, no host wait beyond update's. */
int fftconv_matrix_crossfade_update_pairs(fftconv_matrix_crossfade *h, size_t n_pairs, const uint32_t *pair_out,
                                          const uint32_t *pair_in, const float *responses, size_t response_len,
                                          size_t response_stride);
int fftconv_matrix_crossfade_update_pairs_device(fftconv_matrix_crossfade *h, size_t n_pairs,
                                                 const uint32_t *pair_out, const uint32_t *pair_in,
                                                 const float *d_responses, size_t response_len,
                                                 size_t response_stride, void *hip_stream);
/* |D|: the pairs whose spectra may differ between the two convolvers */
size_t fftconv_matrix_crossfade_diff_pairs(const fftconv_matrix_crossfade *h);
/* the last applied swap: out2 = {pairs transformed, pairs copied}; a whole
 * update gives {inputs * outputs, 0} */
int fftconv_matrix_crossfade_last_patch(const fftconv_matrix_crossfade *h, size_t out2[2]);
int fftconv_matrix_crossfade_reset(fftconv_matrix_crossfade *h);
/* input [inputs][input_len], output [outputs][output_len], host memory. */
int fftconv_matrix_crossfade_process(fftconv_matrix_crossfade *h, const float *input, size_t input_len,
                                     float *output, size_t output_len);
/* device memory, stream-ordered: max_buffer_size samples of input i at d_input +
 * i * in_stride, output_len samples of output o at d_output + o * out_stride. */
int fftconv_matrix_crossfade_process_device(fftconv_matrix_crossfade *h, const float *d_input, size_t in_stride,
                                            float *d_output, size_t out_stride, size_t output_len,
                                            void *hip_stream);
/* `steps` consecutive process_device calls; the same bits as the separate calls. */
int fftconv_matrix_crossfade_process_device_steps(fftconv_matrix_crossfade *h, const float *d_input,
                                                  size_t in_stride, size_t in_step, float *d_output,
                                                  size_t out_stride, size_t out_step, size_t output_len,
                                                  size_t steps, void *hip_stream);
int fftconv_matrix_crossfade_is_crossfading(const fftconv_matrix_crossfade *h); /* :85-92, 1/0 */
fftconv_matrix_crossfade *fftconv_matrix_crossfade_clone(const fftconv_matrix_crossfade *h);
void fftconv_matrix_crossfade_destroy(fftconv_matrix_crossfade *h);
int fftconv_matrix_crossfade_synchronize(fftconv_matrix_crossfade *h);
size_t fftconv_matrix_crossfade_inputs(const fftconv_matrix_crossfade *h);
size_t fftconv_matrix_crossfade_outputs(const fftconv_matrix_crossfade *h);
/* tests and A/B runs: on = 0 makes every call of this handle take the
 * composition path (default 1); a clone inherits the setting. */
int fftconv_matrix_crossfade_set_fused(fftconv_matrix_crossfade *h, int on);
/* the path (0, 1 or 2 above) the next process() would take, a pending
 * response included */
int fftconv_matrix_crossfade_path(const fftconv_matrix_crossfade *h);

/* ---- SparseMatrixCrossfadeConvolver: crossfaded sparse matrix switching ----
 * A sparse matrix crossfade has I inputs, O outputs and N >= 1 listed pairs,
 * strictly ascending in (o, i).  It behaves as N reference
 * CrossfadeConvolver<FFTConvolver> instances (src/crossfade_convolver.rs:3-105),
 * one per listed pair, all created and updated together with the same lengths:
 * instance n processes input i_n, output o is the sum of the instances listed
 * for it; an output without pairs is 0.0 for every sample of every call, inside
 * a fade too.  The crossfaders run in lockstep: one Crossfader, one pending
 * response.  The device mixes the per-output sums, mix(sum a, sum b): equal to
 * the definition within f32 rounding, not bitwise; in hold and Reached samples
 * the mix returns a or b unchanged.  The pattern is fixed for the life of the
 * handle.
 * Everything fftconv_matrix_crossfade_* mirrors from the reference carries over
 * word for word: new / init (init = new(sparse init(...), response_len,
 * max_block_size, response_len)), update (idle: swap at once; fading: stored
 * zero-padded and applied by the first process() after the fade), process
 * advancing both convolvers by max_buffer_size, reset =
 * FFTCONV_E_UNIMPLEMENTED, and the departures (non-finite samples are outside
 * the contract; an update is an update of the whole set).  Row n of `responses`
 * is pair n in list order; response_stride 0 = one response for all.  Errors are
 * those of fftconv_matrix_sparse_init and fftconv_matrix_crossfade_*; no entry
 * point allocates or waits on the host beyond what the dense crossfade's does.
 * Paths (fftconv_matrix_sparse_crossfade_path): 0 composition (A and B as two
 * plain sparse matrices, then the mix kernel), 1 fused with both convolvers
 * live, 2 fused with one convolver idle -- chosen by the handle's state only,
 * exactly as fftconv_matrix_crossfade chooses them ("in step" is its rule), and
 * every path computes the same bits.  Every block size 32..8192 runs fused.
 * Order of summation (part of the contract): per live convolver
 * fftconv_matrix_sparse's, unchanged; then the mix as the dense crossfade
 * applies it.  So (1) a fused call equals the composition call bit for bit;
 * (2) output o is bit-identical, call by call through any script of updates and
 * calls, to the single output of a dense fftconv_matrix_crossfade with k_o
 * inputs that holds h[pair e], is fed x[i_e] and has the same
 * max_response_length, max_buffer_size and crossfade_samples; (3) an output's
 * bits depend only on its own pair list and the inputs it names: a pattern split
 * by outputs over several handles gives identical rows; (4)
 * process_device_steps equals the separate calls.
 * update_pairs is update(R') bit for bit in outputs and in state: R', the base
 * set, len', the merge rules during a fade, the one FFTCONV_E_UNSUPPORTED case
 * and the bookkeeping of D are those of fftconv_matrix_crossfade_update_pairs
 * with "pair" = a listed pair.  The list is (pair_out[n], pair_in[n]), strictly
 * ascending in (o, i); every entry must belong to the pattern -- one that does
 * not is FFTCONV_E_INVALID ("pair (o, i) is not in the pattern"), the handle
 * unchanged.  diff_pairs and last_patch count listed pairs; a whole update
 * gives {N, 0}. */
fftconv_matrix_sparse_crossfade *fftconv_matrix_sparse_crossfade_init(int device, size_t inputs, size_t outputs,
                                                                      size_t pairs, const uint32_t *pair_out,
                                                                      const uint32_t *pair_in, const float *responses,
                                                                      size_t response_len, size_t response_stride,
                                                                      size_t max_block_size,
                                                                      size_t max_response_length);
/* `convolver` is cloned (the caller keeps ownership of its handle). */
fftconv_matrix_sparse_crossfade *fftconv_matrix_sparse_crossfade_new(const fftconv_matrix_sparse *convolver,
                                                                     size_t max_response_length,
                                                                     size_t max_buffer_size,
                                                                     size_t crossfade_samples);
int fftconv_matrix_sparse_crossfade_update(fftconv_matrix_sparse_crossfade *h, const float *responses,
                                           size_t response_len, size_t response_stride);
int fftconv_matrix_sparse_crossfade_update_device(fftconv_matrix_sparse_crossfade *h, const float *d_responses,
                                                  size_t response_len, size_t response_stride, void *hip_stream);
int fftconv_matrix_sparse_crossfade_update_pairs(fftconv_matrix_sparse_crossfade *h, size_t n_pairs,
                                                 const uint32_t *pair_out, const uint32_t *pair_in,
                                                 const float *responses, size_t response_len,
                                                 size_t response_stride);
int fftconv_matrix_sparse_crossfade_update_pairs_device(fftconv_matrix_sparse_crossfade *h, size_t n_pairs,
                                                        const uint32_t *pair_out, const uint32_t *pair_in,
                                                        const float *d_responses, size_t response_len,
                                                        size_t response_stride, void *hip_stream);
/* |D|, in listed pairs */
size_t fftconv_matrix_sparse_crossfade_diff_pairs(const fftconv_matrix_sparse_crossfade *h);
/* the last applied swap: out2 = {pairs transformed, pairs copied}; a whole update gives {pairs, 0} */
int fftconv_matrix_sparse_crossfade_last_patch(const fftconv_matrix_sparse_crossfade *h, size_t out2[2]);
int fftconv_matrix_sparse_crossfade_reset(fftconv_matrix_sparse_crossfade *h);
/* input [inputs][input_len], output [outputs][output_len], host memory. */
int fftconv_matrix_sparse_crossfade_process(fftconv_matrix_sparse_crossfade *h, const float *input, size_t input_len,
                                            float *output, size_t output_len);
/* device memory, stream-ordered, as fftconv_matrix_crossfade_process_device */
int fftconv_matrix_sparse_crossfade_process_device(fftconv_matrix_sparse_crossfade *h, const float *d_input,
                                                   size_t in_stride, float *d_output, size_t out_stride,
                                                   size_t output_len, void *hip_stream);
/* `steps` consecutive process_device calls; the same bits as the separate calls. */
int fftconv_matrix_sparse_crossfade_process_device_steps(fftconv_matrix_sparse_crossfade *h, const float *d_input,
                                                         size_t in_stride, size_t in_step, float *d_output,
                                                         size_t out_stride, size_t out_step, size_t output_len,
                                                         size_t steps, void *hip_stream);
int fftconv_matrix_sparse_crossfade_is_crossfading(const fftconv_matrix_sparse_crossfade *h); /* 1/0 */
fftconv_matrix_sparse_crossfade *fftconv_matrix_sparse_crossfade_clone(const fftconv_matrix_sparse_crossfade *h);
void fftconv_matrix_sparse_crossfade_destroy(fftconv_matrix_sparse_crossfade *h);
int fftconv_matrix_sparse_crossfade_synchronize(fftconv_matrix_sparse_crossfade *h);
size_t fftconv_matrix_sparse_crossfade_inputs(const fftconv_matrix_sparse_crossfade *h);
size_t fftconv_matrix_sparse_crossfade_outputs(const fftconv_matrix_sparse_crossfade *h);
size_t fftconv_matrix_sparse_crossfade_pairs(const fftconv_matrix_sparse_crossfade *h);
/* on = 0: every call of this handle takes the composition path (default 1) */
int fftconv_matrix_sparse_crossfade_set_fused(fftconv_matrix_sparse_crossfade *h, int on);
/* the path (0, 1 or 2) the next process() would take, a pending response included */
int fftconv_matrix_sparse_crossfade_path(const fftconv_matrix_sparse_crossfade *h);

/* ---- MatrixLookaheadCrossfadeConvolver: the crossfaded matrix with far-row windows ----
 * fftconv_matrix_crossfade's definition, unchanged: I*O reference
 * CrossfadeConvolver<FFTConvolver> instances in lockstep, one Crossfader, one
 * pending response, the mix applied to the per-output sums, reset =
 * FFTCONV_E_UNIMPLEMENTED, and the matrix's two departures.  The only
 * difference: the two convolvers A and B are lookahead matrices
 * (fftconv_matrix_lookahead), so each convolver's order of summation is that
 * handle's -- pre = near + far, the same Pn / Pf rules, contiguous far row
 * groups, ascending adds -- and a live convolver's far rows are summed once every
 * fftconv_matrix_lookahead_period() blocks.  Blocks 32..512; a larger block is
 * FFTCONV_E_UNSUPPORTED (use fftconv_matrix_crossfade).
 * Every entry point mirrors fftconv_matrix_crossfade_* word for word, update_pairs
 * and its errors included; `new` clones a fftconv_matrix_lookahead handle, its
 * windows and its block count too.
 * Windows, all host bookkeeping: (1) any swap into the convolver that is not the
 * crossfader's target -- update, update_pairs, or the pending response applied by
 * process() -- invalidates that convolver's windows, as
 * fftconv_matrix_lookahead_update does; it sums its far rows in full until its
 * outputs have anchored again, at most period - 1 blocks each.  (2) On the fused
 * paths a convolver the crossfader has Reached away from is idle: it keeps its
 * delay line, input buffer and block count, makes no anchor and reads no window,
 * and its windows stay invalid for as long as it idles.  So no block ever reads a
 * window row that was anchored before the last swap into its convolver or across
 * an idle spell, and the bits do not depend on whether a far sum came from a
 * window.
 * Paths (fftconv_matrix_lookahead_crossfade_path): 0 composition (A and B as two
 * lookahead matrices, then the mix kernel), 1 fused with both convolvers live, 2
 * fused with one idle; "in step" is fftconv_matrix_crossfade's rule and equal
 * block counts.  Every path computes the same bits, so: a fused call equals the
 * composition call; windows on equals fftconv_matrix_lookahead_crossfade_set_windows(h, 0);
 * a handle that was never updated equals a fftconv_matrix_lookahead over the
 * same calls; once a fade has ended every sample equals a fftconv_matrix_lookahead
 * that received the same update at the same call boundary; a matrix split by
 * outputs gives identical rows; process_device_steps equals the separate calls. */
fftconv_matrix_lookahead_crossfade *fftconv_matrix_lookahead_crossfade_init(int device, size_t inputs, size_t outputs,
                                                                            const float *responses, size_t response_len,
                                                                            size_t response_stride, size_t max_block_size,
                                                                            size_t max_response_length);
/* `convolver` is cloned (the caller keeps ownership of its handle). */
fftconv_matrix_lookahead_crossfade *fftconv_matrix_lookahead_crossfade_new(const fftconv_matrix_lookahead *convolver,
                                                                           size_t max_response_length,
                                                                           size_t max_buffer_size,
                                                                           size_t crossfade_samples);
int fftconv_matrix_lookahead_crossfade_update(fftconv_matrix_lookahead_crossfade *h, const float *responses,
                                              size_t response_len, size_t response_stride);
int fftconv_matrix_lookahead_crossfade_update_device(fftconv_matrix_lookahead_crossfade *h, const float *d_responses,
                                                     size_t response_len, size_t response_stride, void *hip_stream);
int fftconv_matrix_lookahead_crossfade_update_pairs(fftconv_matrix_lookahead_crossfade *h, size_t n_pairs,
                                                    const uint32_t *pair_out, const uint32_t *pair_in,
                                                    const float *responses, size_t response_len, size_t response_stride);
int fftconv_matrix_lookahead_crossfade_update_pairs_device(fftconv_matrix_lookahead_crossfade *h, size_t n_pairs,
                                                           const uint32_t *pair_out, const uint32_t *pair_in,
                                                           const float *d_responses, size_t response_len,
                                                           size_t response_stride, void *hip_stream);
/* |D|, as fftconv_matrix_crossfade_diff_pairs */
size_t fftconv_matrix_lookahead_crossfade_diff_pairs(const fftconv_matrix_lookahead_crossfade *h);
/* the last applied swap: out2 = {pairs transformed, pairs copied}; a whole update gives {I*O, 0} */
int fftconv_matrix_lookahead_crossfade_last_patch(const fftconv_matrix_lookahead_crossfade *h, size_t out2[2]);
int fftconv_matrix_lookahead_crossfade_reset(fftconv_matrix_lookahead_crossfade *h);
/* input [inputs][input_len], output [outputs][output_len], host memory. */
int fftconv_matrix_lookahead_crossfade_process(fftconv_matrix_lookahead_crossfade *h, const float *input, size_t input_len,
                                               float *output, size_t output_len);
/* device memory, stream-ordered, as fftconv_matrix_crossfade_process_device */
int fftconv_matrix_lookahead_crossfade_process_device(fftconv_matrix_lookahead_crossfade *h, const float *d_input,
                                                      size_t in_stride, float *d_output, size_t out_stride,
                                                      size_t output_len, void *hip_stream);
/* `steps` consecutive process_device calls; the same bits as the separate calls. */
int fftconv_matrix_lookahead_crossfade_process_device_steps(fftconv_matrix_lookahead_crossfade *h, const float *d_input,
                                                            size_t in_stride, size_t in_step, float *d_output,
                                                            size_t out_stride, size_t out_step, size_t output_len,
                                                            size_t steps, void *hip_stream);
int fftconv_matrix_lookahead_crossfade_is_crossfading(const fftconv_matrix_lookahead_crossfade *h); /* 1/0 */
fftconv_matrix_lookahead_crossfade *fftconv_matrix_lookahead_crossfade_clone(const fftconv_matrix_lookahead_crossfade *h);
void fftconv_matrix_lookahead_crossfade_destroy(fftconv_matrix_lookahead_crossfade *h);
int fftconv_matrix_lookahead_crossfade_synchronize(fftconv_matrix_lookahead_crossfade *h);
size_t fftconv_matrix_lookahead_crossfade_inputs(const fftconv_matrix_lookahead_crossfade *h);
size_t fftconv_matrix_lookahead_crossfade_outputs(const fftconv_matrix_lookahead_crossfade *h);
/* on = 0: every call of this handle takes the composition path (default 1) */
int fftconv_matrix_lookahead_crossfade_set_fused(fftconv_matrix_lookahead_crossfade *h, int on);
/* the path (0, 1 or 2) the next process() would take, a pending response included */
int fftconv_matrix_lookahead_crossfade_path(const fftconv_matrix_lookahead_crossfade *h);
/* on = 0: both convolvers sum their far rows in full on every block (default 1; the same bits) */
int fftconv_matrix_lookahead_crossfade_set_windows(fftconv_matrix_lookahead_crossfade *h, int on);
/* the outputs of convolver `which` (0 = A, 1 = B) that anchor when the next
 * block starts; 0 for an idle convolver */
int fftconv_matrix_lookahead_crossfade_anchors(const fftconv_matrix_lookahead_crossfade *h, int which);

/* ---- MatrixTwoStageConvolver: two-stage partitioning for the matrix ----
 * A matrix two-stage convolver (inputs I, outputs O, head block max_block_size,
 * max_response_length L) behaves as I*O reference TwoStageFFTConvolver
 * instances (o, i) (src/fft_convolver.rs:323-526), all created and reset
 * together with the same lengths: instance (o, i) processes input i with the
 * same calls, output o is the sum over i.  Everything in process (:412-495)
 * that is not a convolver -- tail_input_fill, precalculated_pos, the two buffer
 * swaps, the sub-chunk loop -- runs in lockstep, so the handle keeps one copy
 * of those scalars on the host.  The device keeps tail_output0,
 * tail_precalculated0, tail_output and tail_precalculated summed per output
 * ([O][T] each) and tail_input per input ([I][T]): results equal the summed
 * instances within f32 rounding, not bitwise.
 * Stages (:340-406), T = fftconv_compute_tail_block_size(max_block_size, L),
 * each pair's response zero-extended to L first; each stage is a matrix as
 * fftconv_matrix_*:
 *   head   padded_ir[0 .. min(L, T)],               block max_block_size
 *   tail0  padded_ir[T .. T + min(L - T, T)],       block max_block_size, only when L > T
 *   tail   padded_ir[2T .. L],                      block T,              only when L > 2T
 * An absent stage contributes nothing and is skipped (the reference's Default
 * convolver outputs zeros).
 * The plain matrix's departures carry over: non-finite samples are outside the
 * parity contract; outputs do not depend on `outputs`, so a matrix split by
 * outputs over several handles computes bit-identical rows.
 * Mirrored from the reference:
 *  - process: len > max_block_size is FFTCONV_E_INVALID (the assert at :414).
 *    A head block size that does not divide T runs tail_input past its end
 *    (:459-460): FFTCONV_E_INVALID at the call where the reference panics.
 *  - update is todo!() (:408-410): FFTCONV_E_UNIMPLEMENTED, handle unchanged.
 *  - reset: :497-511.  clone: a deep copy, mid-period state included.
 * Limits: 32 <= next_power_of_two(max_block_size) <= 8192 as for the plain
 * matrix, and T <= 8192 (the tail is a matrix of block T), else
 * FFTCONV_E_UNSUPPORTED before anything is allocated (head 512 / L 262,144
 * gives T 16,384; head 64 and head 256 / L 262,144 are supported).  inputs == 0,
 * outputs == 0 or response_len > L is FFTCONV_E_INVALID; init returns NULL on
 * error (fftconv_last_error).  Pairs and strides as fftconv_matrix_*.
 * Everything runs on one stream, in stream order; the tail's block-T
 * convolution at the end of a period is enqueued inline, where the reference
 * runs it (:479-486), so the call that ends a period carries it.
 * Paths (fftconv_matrix_twostage_path) -- both compute the same bits:
 *   0  composition: head, then per sub-chunk one small kernel (the sums of
 *      :438-454 and the copy into tail_input), tail0 on each completed head
 *      block, the swaps and the tail at the end of the period.
 *   1  fused: head, the sub-chunk and tail0 in the plain matrix's two launches
 *      -- one forward transform per input for both delay lines, every delay-
 *      line row streamed once for both responses.  Taken when the call is
 *      aligned (len == max_block_size, a power of two; tail_input_fill a
 *      multiple of it; the head's input buffer empty), tail0 exists and head
 *      and tail0 have equal segment counts. */
fftconv_matrix_twostage *fftconv_matrix_twostage_init(int device, size_t inputs, size_t outputs,
                                                      const float *responses, size_t response_len,
                                                      size_t response_stride, size_t max_block_size,
                                                      size_t max_response_length);
/* :408-410: FFTCONV_E_UNIMPLEMENTED */
int fftconv_matrix_twostage_update(fftconv_matrix_twostage *h, const float *responses, size_t response_len,
                                   size_t response_stride);
int fftconv_matrix_twostage_reset(fftconv_matrix_twostage *h); /* :497-511 */
/* input [inputs][len], output [outputs][len], host memory. */
int fftconv_matrix_twostage_process(fftconv_matrix_twostage *h, const float *input, float *output, size_t len);
/* device memory, stream-ordered: input i at d_input + i * in_stride, output o
 * at d_output + o * out_stride (strides in floats). */
int fftconv_matrix_twostage_process_device(fftconv_matrix_twostage *h, const float *d_input, size_t in_stride,
                                           float *d_output, size_t out_stride, size_t len, void *hip_stream);
/* `steps` consecutive process_device calls; the same bits as the separate calls. */
int fftconv_matrix_twostage_process_device_steps(fftconv_matrix_twostage *h, const float *d_input,
                                                 size_t in_stride, size_t in_step, float *d_output,
                                                 size_t out_stride, size_t out_step, size_t len, size_t steps,
                                                 void *hip_stream);
fftconv_matrix_twostage *fftconv_matrix_twostage_clone(const fftconv_matrix_twostage *h);
void fftconv_matrix_twostage_destroy(fftconv_matrix_twostage *h);
int fftconv_matrix_twostage_synchronize(fftconv_matrix_twostage *h);
size_t fftconv_matrix_twostage_inputs(const fftconv_matrix_twostage *h);
size_t fftconv_matrix_twostage_outputs(const fftconv_matrix_twostage *h);
size_t fftconv_matrix_twostage_tail_block_size(const fftconv_matrix_twostage *h);
/* tests and A/B runs: on = 0 makes every call of this handle take the
 * composition path (default 1); a clone inherits the setting. */
int fftconv_matrix_twostage_set_fused(fftconv_matrix_twostage *h, int on);
/* the path (0 or 1 above) the next process() of `len` samples would take */
int fftconv_matrix_twostage_path(const fftconv_matrix_twostage *h, size_t len);

/* ---- SparseMatrixTwoStageConvolver: two-stage partitioning over a listed pair set ----
 * A sparse two-stage matrix has I inputs, O outputs and N >= 1 pairs (o_n, i_n),
 * strictly ascending in (o, i) as for fftconv_matrix_sparse_init, a head block
 * max_block_size and max_response_length L.  It behaves as N reference
 * TwoStageFFTConvolver instances (src/fft_convolver.rs:323-526), one per listed
 * pair, all created and reset together with the same lengths: instance n
 * processes input i_n with the same calls, output o is the sum of the
 * instances listed for it.  An output without pairs is 0.0 for every sample of
 * every call; an input that no pair reads is accepted and ignored; the pattern
 * is fixed for the life of the handle.
 * Stages, T, absent stages, the host's single copy of {tail_input_fill,
 * precalculated_pos} and the two buffer swaps are the dense two-stage matrix's
 * (above): tail_output0 / tail_precalculated0 / tail_output /
 * tail_precalculated summed per output [O][T], tail_input per input [I][T].
 * Each stage is a SPARSE matrix (fftconv_matrix_sparse_*) over the same pattern:
 *   head   padded_ir[0 .. min(L, T)],               block max_block_size
 *   tail0  padded_ir[T .. T + min(L - T, T)],       block max_block_size, only when L > T
 *   tail   padded_ir[2T .. L],                      block T,              only when L > 2T
 * Order of summation (part of the contract): each stage's is the sparse
 * matrix's -- P_o = matrix_parts_rule(k_o, active) per output, rows flattened
 * pair-major in list order, the row-0 terms in ascending e -- and the sums
 * ((y / N + ovl) + tail_precalculated0) + tail_precalculated are in the dense
 * two-stage's order.  So
 *  1. output o is bit-identical to the single output of a dense
 *     fftconv_matrix_twostage with k_o inputs that holds h[pair e] and is fed
 *     x[i_e] in list order;
 *  2. an output's bits depend on nothing outside its own pair list: a pattern
 *     split by outputs over several handles computes identical rows;
 *  3. both paths below compute the same bits.
 * Mirrored from the reference, as the dense handle: len > max_block_size is
 * FFTCONV_E_INVALID (:414); a head block that does not divide T is
 * FFTCONV_E_INVALID at the call where the reference panics (:459-460); update
 * is FFTCONV_E_UNIMPLEMENTED with the handle unchanged (:408-410).  Pattern
 * errors as fftconv_matrix_sparse_init (FFTCONV_E_INVALID); response_len > L is
 * FFTCONV_E_INVALID; a block outside 32..8192 or T > 8192 is
 * FFTCONV_E_UNSUPPORTED before anything is allocated.  A failed launch between
 * the stages makes every later call fail (FFTCONV_E_DEVICE).  init returns NULL
 * on error (fftconv_last_error).  Responses are in pair-list order, row n at
 * responses + n * response_stride; stride 0 = one response for every pair.
 * Streams and signatures as fftconv_matrix_twostage_*; the call that ends a
 * period carries the tail's block-T convolution inline.
 * Paths (fftconv_matrix_sparse_twostage_path) -- both compute the same bits:
 *   0  composition: the three sparse stages and the dense handle's sub-chunk
 *      kernel.
 *   1  fused: head, the sub-chunk and tail0 in the sparse matrix's two launches
 *      -- one forward transform per input for both delay lines, every delay-
 *      line row and pattern entry loaded once for both responses.  Taken under
 *      the dense handle's conditions (an aligned call, tail0 exists, equal
 *      segment counts) and equal MAC plans of head and tail0.
 * Out of scope: update / update_pairs, changing the pattern after init, T >
 * 8192, a crossfade over two-stage matrices. */
fftconv_matrix_sparse_twostage *fftconv_matrix_sparse_twostage_init(int device, size_t inputs, size_t outputs,
                                                                    size_t pairs, const uint32_t *pair_out,
                                                                    const uint32_t *pair_in, const float *responses,
                                                                    size_t response_len, size_t response_stride,
                                                                    size_t max_block_size, size_t max_response_length);
/* :408-410: FFTCONV_E_UNIMPLEMENTED */
int fftconv_matrix_sparse_twostage_update(fftconv_matrix_sparse_twostage *h, const float *responses,
                                          size_t response_len, size_t response_stride);
int fftconv_matrix_sparse_twostage_reset(fftconv_matrix_sparse_twostage *h); /* :497-511 */
/* input [inputs][len], output [outputs][len], host memory. */
int fftconv_matrix_sparse_twostage_process(fftconv_matrix_sparse_twostage *h, const float *input, float *output,
                                           size_t len);
/* device memory, stream-ordered: input i at d_input + i * in_stride, output o
 * at d_output + o * out_stride (strides in floats). */
int fftconv_matrix_sparse_twostage_process_device(fftconv_matrix_sparse_twostage *h, const float *d_input,
                                                  size_t in_stride, float *d_output, size_t out_stride, size_t len,
                                                  void *hip_stream);
/* `steps` consecutive process_device calls; the same bits as the separate calls. */
int fftconv_matrix_sparse_twostage_process_device_steps(fftconv_matrix_sparse_twostage *h, const float *d_input,
                                                        size_t in_stride, size_t in_step, float *d_output,
                                                        size_t out_stride, size_t out_step, size_t len, size_t steps,
                                                        void *hip_stream);
fftconv_matrix_sparse_twostage *fftconv_matrix_sparse_twostage_clone(const fftconv_matrix_sparse_twostage *h);
void fftconv_matrix_sparse_twostage_destroy(fftconv_matrix_sparse_twostage *h);
int fftconv_matrix_sparse_twostage_synchronize(fftconv_matrix_sparse_twostage *h);
size_t fftconv_matrix_sparse_twostage_inputs(const fftconv_matrix_sparse_twostage *h);
size_t fftconv_matrix_sparse_twostage_outputs(const fftconv_matrix_sparse_twostage *h);
size_t fftconv_matrix_sparse_twostage_pairs(const fftconv_matrix_sparse_twostage *h);
size_t fftconv_matrix_sparse_twostage_tail_block_size(const fftconv_matrix_sparse_twostage *h);
/* tests and A/B runs: on = 0 makes every call of this handle take the
 * composition path (default 1); a clone inherits the setting. */
int fftconv_matrix_sparse_twostage_set_fused(fftconv_matrix_sparse_twostage *h, int on);
/* the path (0 or 1 above) the next process() of `len` samples would take */
int fftconv_matrix_sparse_twostage_path(const fftconv_matrix_sparse_twostage *h, size_t len);

#ifdef __cplusplus
}
#endif

#endif /* FFTCONV_H */

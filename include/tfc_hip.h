/*
 * tfc_hip.h — C ABI of the MI355X (gfx950) entropy-coding + transform hot path.
 *
 * This is the drop-in boundary: every entry point replaces one CPU op kernel
 * (or one stock-TF composition) of tensorflow/compression; the reference
 * interface it stands in for is cited as file:line under /root/reference/
 * tensorflow_compression/.  Plain pointers and sizes only — no torch / TF types.
 *
 * Conventions
 *   - Pointers marked DEV are HIP device pointers, HOST are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *     are asynchronous on that stream unless the comment says "synchronises".
 *   - Return value 0 = OK; non-zero = InvalidArgument-class failure whose text
 *     (same substrings the reference's OP_REQUIRES messages carry) is returned
 *     by tfc_last_error() on the calling thread.
 *   - A handle must not be used from two host threads at once (the reference
 *     handles are single-consumer too, cc/ops/range_coder_ops.cc:94-95).
 */
#ifndef TFC_HIP_H_
#define TFC_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfc_tables tfc_tables;
typedef struct tfc_encoder tfc_encoder;
typedef struct tfc_decoder tfc_decoder;

/* Library identity; bumps when the ABI changes (compression_amd/_lib.py refuses a library whose
 * version is not the one it was written against).  2: round-3 ABI (per-handle modes, *_many entry
 * points, stream-ordered finalize, CU-masked streams). */
#define TFC_ABI_VERSION 2
int tfc_abi_version(void);
/* Text of the last failure on this thread ("" if none). */
const char* tfc_last_error(void);

/* Diagnostics for bench.py: when enabled, the library brackets its main kernels
 * ("enc_kernel", "dec_kernel", "gdn_forward", ...) with HIP events on the
 * launch stream; tfc_profile_query returns the accumulated time and launch
 * count of one kernel name (synchronises on the recorded events).  Enabling
 * resets the counters. */
void tfc_profile_enable(int on);
int tfc_profile_query(const char* kernel, double* total_ms, int64_t* launches);
/* Diagnostics for the tests: encode / decode launches of throughput-mode handles that went to the pipelined
 * kernels (csrc/range_pipe.h) since the library was loaded, and workgroups of the lane-per-stream kernels that
 * ran behind them as the fallback for a job they gave up on (synchronises the device).  Either may be null. */
int tfc_pipe_counters(int64_t* launches, int64_t* fallback_blocks);
/* Diagnostics of the pipelined decoder's chain kernel (csrc/range_pipe.h), first chain wave (streams 0 ... 63) of the
 * last decode launch: its memory phases (one per 16-row block), the phases that requested a new code window, and (index
 * mode) those that requested a new window of row addresses — a window is refilled only when a lane of the wave runs low.
 * Synchronises the device.  Any pointer may be null. */
int tfc_debug_pipe_window(int64_t* phases, int64_t* refills, int64_t* index_refills);
/* A/B and test switch of the pipelined decoder (csrc/range_pipe.h): which table image its chain kernel runs on —
 * 0 by launch (the full image where it fits a CU and the launch's chain waves all find one, else the compact image),
 * 1 the full image (one bit per quotient value), 2 the compact image (every second bound at pair resolution: half the
 * bitmaps, ~10 % more cycles per row) — and how many chain waves share a workgroup's copy of it (0: by launch size).
 * Same symbols either way.  Returns the previous format; the environment (TFC_PIPE_FORMAT = full | pairs,
 * TFC_PIPE_WAVES) sets the initial values. */
int tfc_set_pipe_format(int format, int waves_per_workgroup);

/* Kernel family of a coder handle (no reference counterpart: the reference's ops shard streams over the
 * intra-op thread pool, range_coder_kernels.cc:212-267).  The bytes / symbols produced are identical.
 *   TFC_MODE_LATENCY     one code stream per 64-lane wave: shortest time for one call on an idle GPU
 *                        (elems x ~90 cycles encode, ~160 decode), 15-28 vector instructions per symbol;
 *   TFC_MODE_THROUGHPUT  one code stream per LANE: ~1 instruction per symbol and 64 streams, elems x
 *                        ~400 cycles per call — for callers that keep many independent calls in flight
 *                        on different HIP streams, or code thousands of streams per call;
 *   TFC_MODE_AUTO        by the stream count of the handle (throughput kernels from 4096 streams).
 * Tables the throughput kernels cannot hold (LDS image > 160 KB, rows with zero-width symbols) fall
 * back to the latency kernels.  The process-wide default applies to handles left at TFC_MODE_AUTO;
 * its initial value comes from the environment variable TFC_DEFAULT_MODE = latency | throughput. */
#define TFC_MODE_AUTO 0
#define TFC_MODE_LATENCY 1
#define TFC_MODE_THROUGHPUT 2
int tfc_set_default_mode(int mode);
int tfc_get_default_mode(void);

/* Process-wide hint: 1 = the caller keeps other kernels (the transforms of other batches) in flight beside the coder's,
 * 0 (default) = a coder call has the chip to itself.  Shared: handles of 512 streams and more are created with two
 * waves per SIMD (half the CUs; a convolution workgroup cannot use a CU that hosts a coder wave).  Takes effect for
 * handles created afterwards.  No reference counterpart (TensorFlow's executor owns such placement). */
int tfc_set_chip_shared(int shared);     /* -> the previous value */
/* Device memory the library keeps for reuse: every buffer a call or handle releases goes to per-size free lists instead
 * of back to the driver (hipFreeAsync behind a running kernel holds the calling thread until that kernel ends).
 * tfc_cache_bytes: bytes cached now; tfc_cache_trim: returns the blocks whose last use has completed to the driver
 * (-> bytes released).  TFC_CACHE_LIMIT_MB bounds the cache (default 65536).  No reference counterpart (TensorFlow's
 * allocator owns the ops' scratch memory). */
/* Elementwise passes of the model pipelines (csrc/elementwise.hip), one kernel each; dtype 0 = float32, 1 = bfloat16.
 * tfc_image_to_unit: y[i] = dtype(x[i]) / 255 for uint8 x (models/bls2017.py:164-170, bmshj2018.py:219-224).
 * tfc_unit_to_image: y[i] = saturate_cast<uint8>(round_half_even(dtype(x[i] * 255))) (bls2017.py:186-190).
 * tfc_index_prepare: out[i] = int32(min(max(indexes[i], 0), num_tables - 1)), cast toward zero
 * (continuous_indexed.py:272-296: `_normalize_indexes` and the int32 cast of `_flatten_indexes`, one index range). */
int tfc_image_to_unit(const void* x, void* y, int dtype, int64_t n, void* stream);
int tfc_unit_to_image(const void* x, int dtype, void* y, int64_t n, void* stream);
int tfc_index_prepare(const void* indexes, int dtype, int32_t* out, int64_t n, int num_tables, void* stream);
/* Spatial padding of an NHWC tensor [n, h, w, c] of 2- or 4-byte elements into y [n, top + h + bottom, left + w + right, c]:
 * reflect = 0 zeros, 1 mirror without repeating the edge (tf.pad "CONSTANT" / "REFLECT") — the pre-pad of
 * SignalConv2D's `same_reflect` / pre-padded `same_zeros` modes (python/layers/signal_conv.py:880-893). */
int tfc_pad2d(const void* x, void* y, int elem_bytes, int64_t n, int64_t h, int64_t w, int64_t c, int top, int bottom,
              int left, int right, int reflect, void* stream);
int tfc_cache_bytes(long long* bytes);
int tfc_cache_trim(long long* released);

/* ------------------------------------------------------------------------ */
/* CDF tables                                                               */
/* ------------------------------------------------------------------------ */

/* Validates `lookup` and uploads it in the device layout the coders use.
 * Replaces ScanCDF / IndexCDFVector / IndexCDFMatrix
 * (cc/kernels/range_coder_kernels.cc:101-164): rank 1 = ragged concatenation
 * of rows [+-precision, 0, ..., 1<<precision]; rank 2 = [rows, cols], rows
 * padded with 1<<precision.  Negative precision enables the Elias-gamma
 * escape for that row.  `lookup` is HOST (rank 1: cols ints; rank 2:
 * rows*cols ints).  Synchronises on `stream` for the upload. */
int tfc_tables_create(const int32_t* lookup, int rank, int64_t rows, int64_t cols,
                      void* stream, tfc_tables** out);
int64_t tfc_tables_count(const tfc_tables* t);
void tfc_tables_destroy(tfc_tables* t);

/* ------------------------------------------------------------------------ */
/* Multi-stream range encoder (one independent code stream per handle       */
/* element)                                                                 */
/* ------------------------------------------------------------------------ */

/* CreateRangeEncoder — cc/ops/range_coder_ops.cc:28-67,
 * cc/kernels/range_coder_kernels.cc:484-507.  `streams` = number of elements
 * of the handle shape. */
int tfc_encoder_create(const tfc_tables* tables, int64_t streams, void* stream,
                       tfc_encoder** out);

/* n handles of `streams` streams each with one allocation and one launch (per-handle driver calls and
 * small kernels are a measurable part of a step once the coding calls of a group share a launch);
 * out: HOST tfc_encoder*[n].  Each handle is destroyed on its own. */
int tfc_encoder_create_many(const tfc_tables* tables, int64_t streams, int n, void* stream,
                            tfc_encoder** out);

/* Selects the kernel family (TFC_MODE_*); only before the first encode call on the handle. */
int tfc_encoder_set_mode(tfc_encoder* e, int mode);
/* on = 1: encode calls never synchronise; an "index=… / value=… not in range" failure is recorded
 * on the device and returned by tfc_encoder_finalize / tfc_encoder_status instead of by the encode
 * call that met it (throughput-mode handles only; latency-mode calls validate before coding and
 * always report at once).  After such a failure the handle's streams are meaningless. */
int tfc_encoder_set_deferred_errors(tfc_encoder* e, int on);

/* EntropyEncodeChannel (index == NULL) / EntropyEncodeIndex —
 * cc/ops/range_coder_ops.cc:69-127, cc/kernels/range_coder_kernels.cc:191-272,
 * 290-322.  value/index: DEV int32 [streams, elems] row-major.  Appends to
 * every stream; may be called repeatedly on one handle.  Range errors
 * ("index=… not in range", "value=… not in range"): latency-mode handles run a
 * validation pass before anything is appended and synchronise once to read its
 * result (and the exact output bound); throughput-mode handles code in one
 * kernel and synchronise once afterwards to read the error word, unless
 * tfc_encoder_set_deferred_errors(e, 1). */
int tfc_encoder_encode(tfc_encoder* e, const int32_t* value, const int32_t* index,
                       int64_t elems, void* stream);

/* The same for n independent handles (same tables, same stream count, same elems; value[k] / index[k] of
 * handle k) in ONE launch where the handles use the throughput kernels (TFC_MODE_THROUGHPUT, or
 * TFC_MODE_AUTO with n * streams >= 4096): the hardware overlaps only a handful of kernels however many
 * HIP streams carry them, and a 512-stream call is 8 waves, so independent calls fill the chip only
 * as one grid.  Results are exactly those of n tfc_encoder_encode calls; other handles are coded by such
 * calls one after the other. */
int tfc_encoder_encode_many(int n, tfc_encoder* const* e, const int32_t* const* value,
                            const int32_t* const* index, int64_t elems, void* stream);

/* Fused quantise + encode, channel mode:
 *   sym = int32(rint(y - qoffset[c])) - cdf_offset[c],  c = j mod channels
 * i.e. ContinuousBatchedEntropyModel.compress's prologue
 * (python/entropy_models/continuous_batched.py:370-380) folded into the
 * coder's load.  y: DEV [streams, elems], dtype 0 = float32, 1 = bfloat16,
 * 2 = float16.  qoffset: DEV float32 [channels] or NULL; cdf_offset: DEV int32
 * [channels]. */
int tfc_encoder_encode_quantized(tfc_encoder* e, const void* y, int dtype,
                                 const float* qoffset, const int32_t* cdf_offset,
                                 int64_t channels, int64_t elems, void* stream);

/* Fused quantise + encode, index mode
 * (python/entropy_models/continuous_indexed.py:355-386):
 *   sym = int32(rint(y)) - cdf_offset[index]. */
int tfc_encoder_encode_quantized_indexed(tfc_encoder* e, const void* y, int dtype,
                                         const int32_t* index, const int32_t* cdf_offset,
                                         int64_t elems, void* stream);

/* ... for n independent handles (same tables, same geometry) as ONE coding launch: tfc_encoder_encode_quantized
 * x tfc_encoder_encode_many.  y: HOST array of n DEV pointers.  Handles of the throughput family quantise in
 * an elementwise pass of their own (HBM-bound) and code int32 symbols with the hand-scheduled blocks — the
 * fused call costs what int32 channel mode costs; other handles go one by one. */
int tfc_encoder_encode_quantized_many(int n, tfc_encoder* const* e, const void* const* y, int dtype,
                                      const float* qoffset, const int32_t* cdf_offset,
                                      int64_t channels, int64_t elems, void* stream);
/* ... and in index mode (tfc_encoder_encode_quantized_indexed for n handles): the main latents of several batches
 * of a hyperprior model (continuous_indexed.py:355-386) as one launch.  y, index: HOST arrays of n DEV pointers. */
int tfc_encoder_encode_quantized_indexed_many(int n, tfc_encoder* const* e, const void* const* y, int dtype,
                                              const int32_t* const* index, const int32_t* cdf_offset,
                                              int64_t elems, void* stream);

/* EntropyEncodeFinalize — cc/ops/range_coder_ops.cc:129-135,
 * cc/kernels/range_coder_kernels.cc:274-287 + cc/lib/range_coder.cc:266-307.
 * Flushes every stream, packs the streams back to back and returns the total
 * byte count.  Synchronises. */
int tfc_encoder_finalize(tfc_encoder* e, void* stream, int64_t* total_bytes);

/* The same without any host synchronisation: the packed blob is allocated at the slabs' capacity and
 * the total (= offsets[streams]) stays on the device; tfc_encoder_result is valid afterwards, a
 * decoder can be created on it at once (stream-ordered).  tfc_encoder_status synchronises, returns
 * deferred failures and the total byte count (total_bytes may be NULL). */
int tfc_encoder_finalize_device(tfc_encoder* e, void* stream);
/* ... of n handles: three launches in all where every handle holds one piece from the throughput kernels
 * (what tfc_encoder_encode_many leaves), otherwise handle by handle. */
int tfc_encoder_finalize_device_many(int n, tfc_encoder* const* e, void* stream);
int tfc_encoder_status(tfc_encoder* e, void* stream, int64_t* total_bytes);

/* After finalize: device views of the packed result (owned by the handle):
 * blob DEV uint8 [total_bytes], offsets DEV int64 [streams + 1]. */
int tfc_encoder_result(const tfc_encoder* e, const uint8_t** blob, const int64_t** offsets);
/* Bytes the device blob was allocated with (>= offsets[streams]): what a caller may map before it
 * knows the total (after tfc_encoder_finalize_device). */
int tfc_encoder_capacity(const tfc_encoder* e, int64_t* bytes);
/* After finalize: copies the result out.  dst_on_device selects hipMemcpy
 * direction.  Synchronises when copying to the host. */
int tfc_encoder_read(const tfc_encoder* e, uint8_t* blob_dst, int64_t* offsets_dst,
                     int dst_on_device, void* stream);
void tfc_encoder_destroy(tfc_encoder* e);

/* ------------------------------------------------------------------------ */
/* Multi-stream range decoder                                               */
/* ------------------------------------------------------------------------ */

/* CreateRangeDecoder — cc/ops/range_coder_ops.cc:137-153,
 * cc/kernels/range_coder_kernels.cc:597-619.  blob/offsets describe `streams`
 * byte strings (offsets int64 [streams+1]); src_on_device says where they
 * live.  Host input is copied to the device.  Device input is BORROWED: like
 * the reference, which ref-holds the tensor and reads it in place
 * (range_coder_kernels.cc:475-478; "caller must make sure `source` outlives",
 * cc/lib/range_coder.h:74-77), the buffers must stay valid and unchanged until
 * the decoder is destroyed. */
int tfc_decoder_create(const tfc_tables* tables, const uint8_t* blob, const int64_t* offsets,
                       int64_t streams, int src_on_device, void* stream, tfc_decoder** out);

/* n decoders on the device-resident strings of n finalized encoders (borrowed in place, like
 * tfc_decoder_create with src_on_device = 1): one allocation, one launch; out: HOST tfc_decoder*[n]. */
int tfc_decoder_create_many(const tfc_tables* tables, int n, tfc_encoder* const* from, void* stream,
                            tfc_decoder** out);

/* Selects the kernel family (TFC_MODE_*) of the following decode calls. */
int tfc_decoder_set_mode(tfc_decoder* d, int mode);

/* EntropyDecodeChannel (index == NULL) / EntropyDecodeIndex —
 * cc/ops/range_coder_ops.cc:155-237, cc/kernels/range_coder_kernels.cc:360-429,
 * 449-471.  index DEV int32 [streams, elems] or NULL; out DEV int32
 * [streams, elems].  Continues where the previous decode call stopped. */
int tfc_decoder_decode(tfc_decoder* d, const int32_t* index, int32_t* out, int64_t elems,
                       void* stream);

/* n independent handles in one launch (see tfc_encoder_encode_many); index may be NULL. */
int tfc_decoder_decode_many(int n, tfc_decoder* const* d, const int32_t* const* index,
                            int32_t* const* out, int64_t elems, void* stream);

/* Fused decode + dequantise (continuous_batched.py:416-422 /
 * continuous_indexed.py:411-417):
 *   y = float(sym + cdf_offset[c or index]) + (qoffset ? qoffset[c] : 0)
 * written as `dtype`.  Channel mode when index == NULL (then `channels` is the
 * table count), else index mode (qoffset must be NULL). */
int tfc_decoder_decode_dequantized(tfc_decoder* d, const int32_t* index, void* y, int dtype,
                                   const float* qoffset, const int32_t* cdf_offset,
                                   int64_t channels, int64_t elems, void* stream);

/* ... for n independent handles as ONE coding launch (channel mode; see tfc_encoder_encode_quantized_many).
 * y: HOST array of n DEV pointers. */
int tfc_decoder_decode_dequantized_many(int n, tfc_decoder* const* d, void* const* y, int dtype,
                                        const float* qoffset, const int32_t* cdf_offset,
                                        int64_t channels, int64_t elems, void* stream);
/* ... and in index mode (continuous_indexed.py:388-417 for n handles).  index, y: HOST arrays of n DEV pointers. */
int tfc_decoder_decode_dequantized_indexed_many(int n, tfc_decoder* const* d, const int32_t* const* index,
                                                void* const* y, int dtype, const int32_t* cdf_offset,
                                                int64_t elems, void* stream);

/* EntropyDecodeFinalize — cc/ops/range_coder_ops.cc:239-246,
 * cc/lib/range_coder.h:144-169.  ok: HOST uint8 [streams] (1 = the weak
 * end-of-stream check passed).  Also reports a deferred "index=… not in
 * range" failure of a previous decode call.  Synchronises. */
int tfc_decoder_finalize(tfc_decoder* d, uint8_t* ok, void* stream);
/* The same in two stream-ordered halves: the weak check into ok DEV uint8 [streams] without
 * synchronising, and the deferred index failure (synchronises). */
int tfc_decoder_finalize_device(tfc_decoder* d, uint8_t* ok, void* stream);
/* ... of n handles with the same stream count: ok DEV uint8 [n, streams]. */
int tfc_decoder_finalize_device_many(int n, tfc_decoder* const* d, uint8_t* ok, void* stream);
int tfc_decoder_status(tfc_decoder* d, void* stream);
void tfc_decoder_destroy(tfc_decoder* d);

/* ------------------------------------------------------------------------ */
/* Deprecated single-stream ops                                             */
/* ------------------------------------------------------------------------ */

/* RangeEncode — cc/ops/range_coding_ops.cc:30-90,
 * cc/kernels/range_coding_kernels.cc:175-275 (+ MergeAxes,
 * range_coding_kernels_util.cc:34-91).  data DEV int16 with shape
 * data_shape[nd]; cdf DEV int32 with shape cdf_shape[nd+1], broadcastable to
 * data_shape + [width].  Returns the encoded string in a malloc'ed HOST buffer
 * (*out, *out_len) which the caller frees with tfc_free().  Synchronises. */
int tfc_range_encode(const int16_t* data, const int64_t* data_shape, int nd,
                     const int32_t* cdf, const int64_t* cdf_shape, int nc,
                     int precision, int debug_level, void* stream,
                     uint8_t** out, int64_t* out_len);

/* RangeDecode — cc/ops/range_coding_ops.cc:92-124,
 * cc/kernels/range_coding_kernels.cc:277-379.  encoded HOST bytes; out DEV
 * int16 of shape out_shape[nd]. */
int tfc_range_decode(const uint8_t* encoded, int64_t encoded_len, const int64_t* out_shape,
                     int nd, const int32_t* cdf, const int64_t* cdf_shape, int nc,
                     int precision, int debug_level, void* stream, int16_t* out);

/* Deprecated UnboundedIndexRangeEncode / UnboundedIndexRangeDecode —
 * cc/kernels/unbounded_index_range_coding_kernels.cc:146-249, 259-367 (checks :54-143).  ONE stream for
 * the whole tensor: element i uses row index[i] of cdf DEV int32 [rows, width] (the first cdf_size[row]
 * entries are the table), is shifted by offset[row], and values outside [0, cdf_size - 2) are coded as the
 * row's last symbol followed by a variable-length code in `overflow_width`-bit digits.  data / index /
 * out DEV int32 with `total` elements; cdf_size, offset DEV int32 [rows].  debug_level 1 validates index,
 * cdf_size and the tables (same messages as the reference).  Encode returns a malloc'ed HOST buffer the
 * caller frees with tfc_free(); decode takes HOST bytes.  Both synchronise. */
int tfc_unbounded_index_range_encode(const int32_t* data, const int32_t* index, int64_t total,
                                     const int32_t* cdf, int64_t rows, int64_t width,
                                     const int32_t* cdf_size, const int32_t* offset, int precision,
                                     int overflow_width, int debug_level, void* stream, uint8_t** out,
                                     int64_t* out_len);
int tfc_unbounded_index_range_decode(const uint8_t* encoded, int64_t encoded_len, const int32_t* index,
                                     int64_t total, const int32_t* cdf, int64_t rows, int64_t width,
                                     const int32_t* cdf_size, const int32_t* offset, int precision,
                                     int overflow_width, int debug_level, int32_t* out, void* stream);

/* StochasticRound — cc/ops/quantization_ops.cc:21-44, cc/kernels/quantization_kernels.cc:47-96.
 * outputs[i] = floor(inputs[i] / step_size), plus 1 when the i-th draw of ONE xoshiro256+ generator
 * (seeded from `seed` with the C++ standard's seed_seq; 24-bit draws in [0, 1)) is below the fractional
 * part — the same draw for the same flat position as the reference's serial loop, so results are
 * identical for identical seeds.  inputs DEV float32 (dtype 0) / bfloat16 (1) / float16 (2), n elements;
 * seed HOST int32[seed_len]; seed_len 0 seeds from the clock (quantization_kernels.cc:75-81); outputs DEV
 * int32.  Asynchronous on `stream`. */
int tfc_stochastic_round(const void* inputs, int dtype, int64_t n, float step_size,
                         const int32_t* seed, int64_t seed_len, int32_t* outputs, void* stream);

void tfc_free(void* p);

/* ------------------------------------------------------------------------ */
/* Run-length gamma / Rice codec                                            */
/* ------------------------------------------------------------------------ */

/* RunLengthEncode / RunLengthGammaEncode — cc/kernels/run_length_kernels.cc (RunLengthEncodeOp),
 * cc/kernels/run_length_gamma_kernels.cc (RunLengthGammaEncodeOp), bits as cc/lib/bit_coder.cc writes them
 * (LSB-first, last byte zero-padded).  `units` coding units of `unit_len` symbols each, data DEV of dtype 0 int32,
 * 1 float32, 2 bfloat16, 3 float16 (floats are rounded half-to-even, then cast to int32, as tf.round + tf.cast).
 * run_length_code / magnitude_code: a Rice parameter in [0, 31], or negative for the gamma code;
 * RunLengthGammaEncode is (-1, -1, nonzero_runs = 0).  Rice parameters above 31 are rejected (undefined in the
 * reference).  Two calls: _size writes offsets DEV int64 [units + 1] (byte offsets of the strings, the layout of
 * tfc_encoder_result) and *total_bytes HOST — it synchronises once, to size the blob; _write fills blob DEV, which
 * the caller zero-fills beforehand with room for total_bytes + 8 bytes and aligns to 4 bytes.  workspace DEV int64
 * [tfc_run_length_workspace(units, unit_len)] carries the per-tile scans from the first call to the second. */
int64_t tfc_run_length_workspace(int64_t units, int64_t unit_len);
int tfc_run_length_encode_size(const void* data, int dtype, int64_t units, int64_t unit_len, int run_length_code,
                               int magnitude_code, int nonzero_runs, int64_t* workspace, int64_t* offsets,
                               int64_t* total_bytes, void* stream);
int tfc_run_length_encode_write(const void* data, int dtype, int64_t units, int64_t unit_len, int run_length_code,
                                int magnitude_code, int nonzero_runs, const int64_t* workspace,
                                const int64_t* offsets, uint8_t* blob, void* stream);
/* RunLengthDecode / RunLengthGammaDecode — cc/kernels/run_length_kernels.cc (RunLengthDecodeOp),
 * cc/kernels/run_length_gamma_kernels.cc (RunLengthGammaDecodeOp), cc/lib/bit_coder.cc (BitReader).
 * blob DEV (readable 16 bytes past offsets[units]), offsets DEV and host_offsets HOST int64 [units + 1];
 * out DEV [units, unit_len] of out_dtype 0 int32, 1 float32, 2 bfloat16 (zero-filled, then the non-zeros).
 * status DEV int32 [units]: 0 OK, 1 "Out of bits to read.", 2 "Exceeded maximum gamma bit width.",
 * 3 "Decoded past end of tensor.", 4 a Rice value that overflows int32 (undefined in the reference; rejected).
 * Kernel family by mean string length: a lane per string, or a chunk-parallel self-synchronising decode for
 * long strings (TFC_RL_DECODER = lane | chunk forces one; TFC_RL_LONG_BITS, default 16384, is the threshold in
 * bits; TFC_RL_CHUNK_BITS, default 1024, the chunk size; TFC_RL_SYNC_ROUNDS, default 2, the speculative
 * rounds).  The chunked family synchronises. */
int tfc_run_length_decode(const uint8_t* blob, const int64_t* offsets, const int64_t* host_offsets, int64_t units,
                          int64_t unit_len, int run_length_code, int magnitude_code, int nonzero_runs,
                          int out_dtype, void* out, int* status, void* stream);

/* ------------------------------------------------------------------------ */
/* PmfToQuantizedCdf                                                        */
/* ------------------------------------------------------------------------ */

/* cc/ops/pmf_to_cdf_ops.cc:28-57, cc/kernels/pmf_to_cdf_kernels.cc:58-208.
 * pmf DEV float32 [rows, n] -> cdf DEV int32 [rows, n+1]; every symbol >= 1,
 * cdf[:,0] = 0, cdf[:,n] = 1 << precision.  Which of several symbols with EQUAL penalty is adjusted
 * follows the order libstdc++'s std::sort leaves them in (csrc/sort_order.h reproduces its introsort),
 * i.e. the tables of the reference built with libstdc++; the reference itself disclaims portability of
 * that order across standard libraries (pmf_to_cdf_ops.cc:45-49). */
int tfc_pmf_to_quantized_cdf(const float* pmf, int64_t rows, int64_t n, int precision,
                             int32_t* cdf, void* stream);

/* A whole model's range-coding tables in one launch — python/entropy_models/continuous_base.py:217-296
 * (`_build_tables`) from the sampled PMFs on: row r of pmf DEV [rows, stride] holds lengths[r] (DEV int32, >= 1)
 * probabilities; the kernel appends overflow = max(1 - sum(pmf[:length]), 0) (continuous_base.py:277-279; float32, in
 * the fixed order csrc/pmf_to_cdf.hip states), runs PmfToQuantizedCdf (pmf_to_cdf_kernels.cc:159-208) on the
 * length + 1 values and writes [-precision, cdf[0 .. length + 1]] at out[offsets[r]] (offsets DEV int64: the caller's
 * prefix sums of length + 3; out DEV int32 [sum]).  max_length = the largest length (sizes the kernel's LDS). */
int tfc_build_tables(const float* pmf, int64_t rows, int64_t stride, const int32_t* lengths, const int64_t* offsets,
                     int64_t max_length, int precision, int32_t* out, void* stream);
/* The same with the overflow mass of every row given (overflow DEV float32 [rows]; null: as tfc_build_tables): the
 * reference forms max(1 - reduce_sum(p), 0) in the PRIOR's dtype and casts to float32 afterwards
 * (continuous_base.py:277-279), so a float64 / bfloat16 prior's caller sums in that arithmetic itself. */
int tfc_build_tables_overflow(const float* pmf, int64_t rows, int64_t stride, const int32_t* lengths,
                              const int64_t* offsets, int64_t max_length, int precision, const float* overflow,
                              int32_t* out, void* stream);
/* helpers.estimate_tails (python/distributions/helpers.py:29-104) for a deep factorized prior
 * (python/distributions/deep_factorized.py:166-246), whole iteration on the device: for every target t (DEV float32
 * [num_targets]) and channel c, the x where the channel's logits of the cumulative reach t — out DEV [num_targets,
 * channels]; iterations DEV int32 [num_targets] or null.  params DEV [channels, params_per_channel]: the
 * reparameterised MLP weights in the layout of tfc_factorized_bits_forward. */
int tfc_deep_factorized_tails(const float* params, int64_t channels, int64_t params_per_channel, int layers, int width,
                              const float* targets, int num_targets, float* out, int* iterations, void* stream);

/* ------------------------------------------------------------------------ */
/* GDN / IGDN                                                               */
/* ------------------------------------------------------------------------ */

/* GDN.call — python/layers/gdn.py:371-421 with channels_last layout:
 *   u = |x|^alpha (alpha_mode 1) or x^2 (alpha_mode 2); rectify => x = max(x,0) first
 *   n_i = beta_i + sum_j gamma[j,i] u_j
 *   y_i = x_i / n_i^eps  (inverse=0)   or   x_i * n_i^eps (inverse=1)
 * eps_mode 0: eps = 1; 1: eps = 0.5.  x,y DEV [pixels, channels] dtype (0 f32,
 * 1 bf16); beta DEV f32 [channels]; gamma DEV f32 [channels(in j), channels(out i)]. */
int tfc_gdn_forward(const void* x, void* y, int dtype, int64_t pixels, int64_t channels,
                    const float* beta, const float* gamma, int inverse, int rectify,
                    int alpha_mode, int eps_mode, void* stream);

/* Inference form: the kernels' LDS image of (beta, gamma) built ONCE (tfc_gdn_params_create launches the small
 * preparation kernel the plain entry point launches per call) and reused by every tfc_gdn_forward_prepared call
 * while the parameters do not change — python/layers/gdn.py holds beta / gamma as variables, constant outside
 * training.  channels / dtype as for tfc_gdn_forward. */
typedef struct tfc_gdn_params tfc_gdn_params;
int tfc_gdn_params_create(const float* beta, const float* gamma, int64_t channels, int dtype, void* stream,
                          tfc_gdn_params** out);
void tfc_gdn_params_destroy(tfc_gdn_params* p);
int tfc_gdn_forward_prepared(const tfc_gdn_params* params, const void* x, void* y, int64_t pixels,
                             int inverse, int rectify, int alpha_mode, int eps_mode, void* stream);

/* The same layer with general (e.g. learned) exponents — python/layers/gdn.py:345-369 creates alpha
 * (>= 1) and epsilon (>= 1e-6) as scalar parameters when the constructor gets None, and :386-387 /
 * :411-412 then take `inputs ** alpha` and `norm_pool ** epsilon` with tf.pow:
 *   u = x^alpha (rectify => x = max(x,0) first; a negative x gives NaN unless alpha is an integer, as tf.pow does)
 *   y_i = x_i / n_i^epsilon  or  x_i * n_i^epsilon.
 * alpha, epsilon: positive finite host scalars.  Forward only: the gradients of this variant (which include
 * d/dalpha and d/depsilon) are composed from device tensor ops by the host layer, not by this library. */
int tfc_gdn_forward_general(const void* x, void* y, int dtype, int64_t pixels, int64_t channels,
                            const float* beta, const float* gamma, int inverse, int rectify,
                            float alpha, float epsilon, void* stream);

/* Backward of tfc_gdn_forward (the reference relies on TF autodiff).  g = dL/dy.
 * Outputs: dx (dtype) and float32 accumulators dbeta [channels], dgamma
 * [channels, channels] which are ADDED to (caller zeroes them). */
int tfc_gdn_backward(const void* x, const void* g, void* dx, int dtype, int64_t pixels,
                     int64_t channels, const float* beta, const float* gamma, int inverse,
                     int rectify, int alpha_mode, int eps_mode, float* dbeta, float* dgamma,
                     void* stream);

/* ChannelNorm of HiFiC — models/hific/archs.py:214-297 (`_get_moments` :262-273, tf.nn.batch_normalization :258) —
 * with the ReLU / residual add the model puts behind it (archs.py:88-98, 129-154, 201-211), one pass over HBM:
 *   mean_p = sum_c x[p,c] / C;   var_p = sum_c (x[p,c] - mean_p)^2 / (C - 1)      (the UNBIASED variance)
 *   y[p,c] = (x[p,c] - mean_p) * rsqrt(var_p + epsilon) * gamma[c] + beta[c];  relu != 0: y = max(y, 0);
 *   residual != NULL: y += residual[p,c] (after the ReLU).
 * x, residual, y DEV [pixels, channels] dtype (0 f32, 1 bf16), channels innermost; gamma, beta DEV f32 [channels] or
 * NULL (scale=False / center=False: 1 / 0).  Statistics in float32; bf16 is rounded once, on the store.  channels >= 2;
 * epsilon finite and >= 0; pixels == 0 returns 0.  Row sizes that are multiples of 16 bytes up to 4 KB bf16 /
 * 8 KB f32, and odd multiples of 8 bytes (rows go in pairs) up to half that, take 16-byte accesses, any other a
 * wave-per-row kernel.  y leaves non-temporal when x + y exceed 128 MiB
 * (TFC_CNORM_NT=0|1 in the environment: never / always). */
int tfc_channel_norm_forward(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                             int dtype, int64_t pixels, int64_t channels, float epsilon, int relu, void* stream);

/* Backward of tfc_channel_norm_forward without a residual (the reference relies on TF autodiff of archs.py:255-273;
 * the residual branch's gradient is g itself).  With xhat = (x - mean) rstd and g' = g * [y before the ReLU > 0]:
 *   dx = rstd * (g' gamma - sum_c(g' gamma) / C - xhat * sum_c(g' gamma xhat) / (C - 1))
 *   dgamma[c] = sum_p g' xhat;   dbeta[c] = sum_p g'.
 * The tf.stop_gradient(mean) of archs.py:267 removes a term proportional to sum_c (x - mean) = 0: no difference.
 * x, g, dx DEV [pixels, channels] dtype; dgamma, dbeta DEV f32 [channels], WRITTEN (not added to), either may be NULL.
 * The statistics are recomputed from x.  Deterministic: per-wave partial sums are added in a fixed order. */
int tfc_channel_norm_backward(const void* x, const void* g, const float* gamma, const float* beta, void* dx,
                              float* dgamma, float* dbeta, int dtype, int64_t pixels, int64_t channels, float epsilon,
                              int relu, void* stream);

/* ------------------------------------------------------------------------ */
/* LPIPS: the distance head and the max-pool                                */
/* ------------------------------------------------------------------------ */

/* The per-layer distance of LPIPS (Zhang et al. 2018; HiFiC's perceptual loss, models/hific/model.py:840-872, which
 * loads it as a frozen graph: the definition here is the paper's, checked against a float64 evaluation of it).
 * f0, f1 DEV [images, pixels, channels] dtype (0 f32, 1 bf16), channels innermost; w DEV f32 [channels]:
 *   n0 = sqrt(sum_c f0^2), n1 = sqrt(sum_c f1^2) per pixel
 *   d[image] = 1 / pixels * sum_p sum_c w[c] (f0[p,c] / (n0 + epsilon) - f1[p,c] / (n1 + epsilon))^2     DEV f32 [images]
 * One pass: a pixel's two rows stay in registers, and the difference is taken before it is squared (the expanded
 * form cancels where f0 ~ f1).  Rows that are multiples of 16 bytes up to 2 KB take 16-byte accesses, any other a
 * wave-per-pixel kernel.  Deterministic: per-workgroup sums are added in a fixed order, no float atomics.
 * epsilon finite and >= 0; pixels >= 1; images == 0 returns 0. */
int tfc_lpips_distance_forward(const void* f0, const void* f1, const float* w, float* d, int dtype, int64_t images,
                               int64_t pixels, int64_t channels, float epsilon, void* stream);

/* Backward of tfc_lpips_distance_forward.  g DEV f32 [images]; mask bit 0: df0 is wanted, bit 1: df1; a gradient that
 * is not wanted is not written and may be NULL.  df0, df1 DEV [images, pixels, channels] dtype.  With
 * a = 1 / (n0 + epsilon), b = 1 / (n1 + epsilon) and e = 2 g[image] / pixels * w (a f0 - b f1):
 *   df0 =  e a - f0 (f0 . e) a^2 / n0,   df1 = -e b + f1 (f1 . e) b^2 / n1,
 * the second term 0 where the norm is 0: the derivative of f / (|f| + epsilon) written out, which is finite at an
 * all-zero pixel (sqrt's own derivative there is inf * 0).  The norms are recomputed from f0 and f1. */
int tfc_lpips_distance_backward(const float* g, const void* f0, const void* f1, const float* w, void* df0, void* df1,
                                int dtype, int64_t images, int64_t pixels, int64_t channels, float epsilon, int mask,
                                void* stream);

/* Max-pool, window k x k, stride s, no padding: x DEV [n, h, w, c] dtype (0 f32, 1 bf16), y DEV
 * [n, (h - k) / s + 1, (w - k) / s + 1, c] (floor).  A NaN in a window is its maximum, as in torch.  h, w >= k. */
int tfc_maxpool2d_forward(const void* x, void* y, int dtype, int64_t n, int64_t h, int64_t w, int64_t c, int k, int s,
                          void* stream);

/* Backward of tfc_maxpool2d_forward as a gather, no atomics: dx[i] = sum of g over the windows whose maximum element i
 * is, the windows in row-major order, summed in float32.  A window's maximum is found from x again (the forward
 * stores nothing but y); among equal values it is the FIRST in the window's row-major order.  g DEV dtype, the shape
 * of y; dx DEV dtype, the shape of x, WRITTEN. */
int tfc_maxpool2d_backward(const void* x, const void* g, void* dx, int dtype, int64_t n, int64_t h, int64_t w,
                           int64_t c, int k, int s, void* stream);

/* ------------------------------------------------------------------------ */
/* SSIM / multiscale SSIM, one scale per call                               */
/* ------------------------------------------------------------------------ */

/* One scale of tf.image.ssim / tf.image.ssim_multiscale.  The definition is TensorFlow's (tensorflow/python/ops/
 * image_ops_impl.py: _ssim_per_channel, ssim_multiscale), not the reference tree's, which only calls it
 * (models/bls2017.py:295); parity with TensorFlow itself is unpinned, the checker is a float64 evaluation of the
 * formulas below.  x, y DEV [batch, height, width, channels], channels innermost, dtype 0 float32, 1 bfloat16,
 * 2 float16, 3 uint8; a plane is one image's one channel.  taps HOST float32 [filter_size], 1 <= filter_size <= 31: the
 * 1-D window g (the 2-D one is g g^T), applied VALID.  With F that filter, c1 = (k1 max_val)^2, c2 = (k2 max_val)^2:
 *   mu1 = F(x), mu2 = F(y), S = F(x^2 + y^2), P = F(x y)
 *   l = (2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1);   cs = (2 P - 2 mu1 mu2 + c2) / (S - mu1^2 - mu2^2 + c2)
 *   means[plane] = (mean(l cs), mean(cs)) over the (height - n + 1)(width - n + 1) positions     DEV f32 [planes, 2]
 * pooled_x, pooled_y: DEV f32 [planes, ceil(height / 2), ceil(width / 2)] or both NULL: the mean of each 2x2 block of
 * x and y, the last row / column repeated where height / width is odd (the next scale's pair; as a call's x, y it is
 * batch = planes, channels = 1).  Moments are accumulated in float32 on x - c, y - c (c: a pixel of the tile), which
 * leaves the variances and the covariance unchanged.  Deterministic: per-workgroup sums are added in a fixed order, no
 * float atomics.  Arguments are checked before anything is launched.  filter_size 11 runs kernels with the tap count as
 * a compile-time constant (TFC_SSIM_RUNTIME_TAPS=1 in the environment: the general kernels, for comparison). */
int tfc_ssim_scale_forward(const void* x, const void* y, int dtype, int64_t batch, int64_t height, int64_t width,
                           int64_t channels, const float* taps, int filter_size, float c1, float c2, float* means,
                           float* pooled_x, float* pooled_y, void* stream);

/* Backward of tfc_ssim_scale_forward (TensorFlow differentiates the composed ops).  grad_means DEV f32 [planes, 2];
 * grad_pooled_x / grad_pooled_y DEV f32 [planes, ceil(height / 2), ceil(width / 2)] or NULL (no gradient arrives
 * through that pooled image).  grad_x, grad_y DEV f32 [batch, height, width, channels], WRITTEN, either may be NULL:
 *   grad_x = F'(a1) + 2 x F'(b) + y F'(c) + pool'(grad_pooled_x)
 * with a1, b, c the derivatives of sum(grad_means[plane] * (l cs, cs)) / positions with respect to mu1, S and P at
 * every position, F' the window as a FULL correlation (the adjoint of F) and pool' a quarter of the coarser gradient
 * per pixel, the repeated row / column folded onto the last one; likewise grad_y.  The moments are recomputed from
 * x and y: nothing else is saved by the forward call. */
int tfc_ssim_scale_backward(const void* x, const void* y, int dtype, int64_t batch, int64_t height, int64_t width,
                            int64_t channels, const float* taps, int filter_size, float c1, float c2,
                            const float* grad_means, const float* grad_pooled_x, const float* grad_pooled_y,
                            float* grad_x, float* grad_y, void* stream);

/* ------------------------------------------------------------------------ */
/* SignalConv2D (same_zeros, explicit padding, NHWC, non-separable)         */
/* ------------------------------------------------------------------------ */

/* _correlate_down_explicit — python/layers/signal_conv.py:663-690:
 * cross-correlation with zero padding (k/2, (k-1)/2) and stride `stride`;
 * out = ceil(in / stride), first output aligned with the first input.
 * x DEV [N,H,W,Cin] (dtype: 0 f32, 1 bf16), w DEV float32 [kh,kw,Cin,Cout] (HWIO, the
 * layer's `kernel`), bias DEV f32 [Cout] or NULL, y DEV [N,ceil(H/s),ceil(W/s),Cout]
 * (same dtype as x).  activation: 0 none, 1 ReLU (fused).  Cin must be a
 * multiple of 16 or <= 4. */
int tfc_conv2d_down(const void* x, const void* w, const float* bias, void* y, int dtype,
                    int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout,
                    int kh, int kw, int stride, int activation, void* stream);

/* _up_convolve_transpose_explicit — python/layers/signal_conv.py:778-847 with
 * extra_pad_end=True: zero-insertion upsampling by `stride` followed by a true
 * convolution centred at k/2, i.e. y[q*s + phi] = sum_i x[i] * w[phi + (q-i)*s + k/2];
 * out = in * stride.  w is the layer's own HWIO kernel [kh,kw,Cin,Cout]; the
 * library does the phase split.  stride 1 gives the flipped-kernel correlation
 * the reference uses for `corr=False` without upsampling (signal_conv.py:865-870). */
int tfc_conv2d_up(const void* x, const void* w, const float* bias, void* y, int dtype,
                  int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout,
                  int kh, int kw, int stride, int activation, void* stream);

/* The layer with GDN / IGDN as its activation — SignalConv2D(activation=GDN(...)), python/layers/signal_conv.py:948-950
 * applying python/layers/gdn.py:371-421 to the convolution's output, as models/bls2017.py:61-91 and bmshj2018.py build
 * their transforms — in ONE kernel where the convolution kernel that takes the layer holds all output channels of its
 * pixels (the third-generation bfloat16 kernel: transposed 5x5 stride-2 layers and small stride-2 maps, Cout 128 / 192):
 * y = conv(x) + bias rounded to bfloat16, then y / (beta + gamma^T |y|) (inverse = 0) or y * (...) (inverse = 1), alpha =
 * epsilon = 1, no rectification; `gdn` = tfc_gdn_params_create of the layer's (beta, gamma) for bfloat16.  *fused = 1:
 * done; *fused = 0: `y` holds the convolution only (another kernel took the layer) and the caller applies
 * tfc_gdn_forward_prepared to it.  up = 0: tfc_conv2d_down's geometry, 1: tfc_conv2d_up's. */
int tfc_conv2d_gdn(const void* x, const void* w, const float* bias, void* y, int dtype,
                   int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout, int kh,
                   int kw, int stride, int up, const tfc_gdn_params* gdn, int inverse, int* fused,
                   void* stream);

/* Inference: the layer's weights do not change between calls.  Every convolution kernel reads the float32 HWIO kernel
 * as fragments in its own order, packed by a small kernel in front of it (60-90 us, four to nine a model step).
 * tfc_conv2d_weights_key(key) names the VALUE of `w` for the NEXT tfc_conv2d_* call of the calling thread (key != 0,
 * chosen by the caller: one number per distinct weight tensor value, never reused for another): that call packs the
 * fragments once per (key, kernel, geometry) and later calls with the same key reuse them, from any thread or stream.
 * Without a key every call packs (training; the reference has no such notion: TF folds constants in its graph).
 * tfc_conv2d_drop_weights(key) releases them (drains the device first): when the weights changed or the layer dies. */
void tfc_conv2d_weights_key(uint64_t key);
int tfc_conv2d_drop_weights(uint64_t key);

/* Weight gradient of either direction (the reference relies on TF autodiff of
 * signal_conv.py:663-690 / 778-847).  G[t][ca][cb] = sum_{n,q} A[n, q*stride + t - k/2, ca] *
 * B[n, q, cb] with zeros outside A; q runs over B's grid.
 *   analysis  y = tfc_conv2d_down(x, w):  dw = G            with A = x  [n,ha,wa,ca=Cin],  B = dy [n,hb,wb,cb=Cout]
 *   synthesis y = tfc_conv2d_up(x, w):    dw = G transposed with A = dy [n,ha,wa,ca=Cout], B = x  [n,hb,wb,cb=Cin]
 * (transpose = 1 writes dw[t][cb][ca]).  dw DEV f32 [kh,kw,Cin,Cout] is ADDED to.  a, b DEV dtype
 * (0 f32, 1 bf16); channel counts <= 4 or multiples of 32 up to 256.  The INPUT gradient needs no
 * entry point of its own: dx of tfc_conv2d_down is tfc_conv2d_up(dy, w with its channel axes
 * swapped) cropped to the input size, and dx of tfc_conv2d_up is tfc_conv2d_down(dy, same). */
int tfc_conv2d_wgrad(const void* a, const void* b, float* dw, int dtype, int64_t n, int64_t ha,
                     int64_t wa, int64_t ca, int64_t hb, int64_t wb, int64_t cb, int kh, int kw,
                     int stride, int transpose, void* stream);

/* What the host of tfc_conv2d_wgrad would choose over B's grid [n,hb,wb] on a device of `cus` compute units, from the
 * function the launch itself takes it from (the launch reads `cus` from its device).  Host only: nothing is launched
 * and no device is touched (no reference counterpart).  dtype, ca, cb, kh, kw are checked as by the call and fail with
 * the same text, the channel pairs that are not built (a side of 96, 160 or 224) included; an empty problem and
 * cus < 1 are errors.  out HOST int32[7] = tiles_ca, tiles_cb (32-channel tiles of the build; 1 for <= 4 channels),
 * chunks (workgroups per tap; workgroup c takes the 64-pixel stages c, c + chunks, ...), chunk_steps (= ceil(stages /
 * chunks): the most stages one workgroup walks), pixels_in_last_stage, tr (1: the bfloat16 build with row-major
 * stages and transposing LDS reads; 0 under TFC_WGRAD_TR=0, which a process reads once), lds_bytes (one workgroup). */
int tfc_conv2d_wgrad_plan(int dtype, int64_t n, int64_t hb, int64_t wb, int64_t ca, int64_t cb, int kh, int kw,
                          int cus, int32_t* out);

/* ------------------------------------------------------------------------ */
/* SignalConv1D / SignalConv3D (same_zeros, explicit padding, NDHWC)        */
/* ------------------------------------------------------------------------ */

/* _correlate_down_explicit — python/layers/signal_conv.py:663-690 — for rank 3, one stride per axis:
 * y[i] = sum_t x[i*s + t - k/2] * w[t] on each axis (zeros outside x), out = ceil(in / s).
 * x DEV [N,D,H,W,Cin] (dtype: 0 f32, 1 bf16), w DEV float32 [kd,kh,kw,Cin,Cout] (DHWIO, the layer's `kernel`),
 * bias DEV f32 [Cout] or NULL, y DEV [N,ceil(D/sd),ceil(H/sh),ceil(W/sw),Cout] (dtype of x).  activation: 0 none,
 * 1 ReLU (fused).  Cin a multiple of 16, Cout >= 1.  Rank 1 is d = h = 1, kd = kh = 1, sd = sh = 1. */
int tfc_conv3d_down(const void* x, const void* w, const float* bias, void* y, int dtype,
                    int64_t n, int64_t d, int64_t h, int64_t wd, int64_t cin, int64_t cout,
                    int kd, int kh, int kw, int sd, int sh, int sw, int activation, void* stream);

/* _up_convolve_transpose_explicit — python/layers/signal_conv.py:778-847 with extra_pad_end=True — for rank 3:
 * y[q*s + phi] = sum_d x[q - d] * w[d*s + phi + k/2] on each axis, out = in * s.  Run phase by phase: each of the
 * sd*sh*sw output phases only takes the taps it has.  Arguments as tfc_conv3d_down. */
int tfc_conv3d_up(const void* x, const void* w, const float* bias, void* y, int dtype,
                  int64_t n, int64_t d, int64_t h, int64_t wd, int64_t cin, int64_t cout,
                  int kd, int kh, int kw, int sd, int sh, int sw, int activation, void* stream);

/* Weight gradient of either rank-3 direction (the reference relies on TF autodiff of signal_conv.py:663-690 /
 * 778-847), the contract of tfc_conv2d_wgrad per axis: G[t][ca][cb] = sum_{n,q} A[n, q*s + t - k/2, ca] * B[n, q, cb]
 * with zeros outside A; q runs over B's grid [db,hb,wb].  Down: A = x, B = dy; up: A = dy, B = x, transpose = 1 writes
 * dw[t][cb][ca].  dw DEV f32 [kd,kh,kw,Cin,Cout] is WRITTEN (not added to).  a, b DEV dtype (0 f32, 1 bf16); channel
 * counts multiples of 16.  Deterministic: partial sums are added in a fixed order. */
int tfc_conv3d_wgrad(const void* a, const void* b, float* dw, int dtype, int64_t n,
                     int64_t da, int64_t ha, int64_t wa, int64_t ca, int64_t db, int64_t hb, int64_t wb,
                     int64_t cb, int kd, int kh, int kw, int sd, int sh, int sw, int transpose, void* stream);

/* What the host would choose for such calls, from the functions the launches themselves take it from.  Host only:
 * nothing is launched and no device is touched, so a test can pick and assert its shapes from the kernels' own tile and
 * chunk rules (no reference counterpart).  Arguments are checked as by the calls; an empty problem is an error.
 * tfc_conv3d_plan: one image of tfc_conv3d_down (up = 0) / tfc_conv3d_up (up = 1) with cin_k input channels AS THE
 * KERNEL SEES THEM (Cin for bfloat16, 6 Cin for float32's planes) -> out HOST int32[8] = TW, TH (the tile: TH x TW
 * output samples of a phase), NT (32-column tiles per workgroup), nblk (column blocks), tiles_w, tiles_h (per phase
 * and depth slice), phases (launches), lds_bytes (one workgroup's stage).
 * tfc_conv3d_wgrad_plan: tfc_conv3d_wgrad over B's grid [n,db,hb,wb] -> out HOST int32[5] = tiles_ca, tiles_cb (64
 * channels each), chunks (of B's pixels, each summed by one workgroup per tap and tile), chunk_steps (LDS stages of
 * 64 pixels per chunk), pixels_in_last_chunk. */
int tfc_conv3d_plan(int up, int64_t d, int64_t h, int64_t wd, int64_t cin_k, int64_t cout,
                    int kd, int kh, int kw, int sd, int sh, int sw, int32_t* out);
int tfc_conv3d_wgrad_plan(int64_t n, int64_t db, int64_t hb, int64_t wb, int64_t ca, int64_t cb,
                          int kd, int kh, int kw, int32_t* out);

/* ------------------------------------------------------------------------ */
/* Training-time entropy bottleneck (deep factorized prior), fused          */
/* ------------------------------------------------------------------------ */

/* ContinuousBatchedEntropyModel.__call__(training=True) with a NoisyDeepFactorized prior and
 * expected_grads=False — python/entropy_models/continuous_batched.py:291-322,
 * python/ops/math_ops.py:157-216, python/distributions/uniform_noise.py:117-156,
 * python/distributions/deep_factorized.py:166-194:
 *   y_hat = y + noise;  log p = log(c(y_hat + .5) - c(y_hat - .5)),  c = sigmoid(logits(.));
 *   bits[u] = -sum over unit u of log p / ln 2.
 * y, noise (or NULL: y_hat = y), y_hat DEV [units, elems] dtype (0 f32, 1 bf16), channels
 * innermost (elems % channels == 0, channels <= 512).  The per-channel MLP has `layers` layers
 * 1 -> width -> ... -> 1; params DEV f32 [channels, P] holds the REPARAMETERISED values
 * (softplus(matrix), bias, tanh(factor)) per channel: layer 0 m[W] b[W] a[W]; middle layers
 * m[W][W] (row = output) b[W] a[W]; last layer m[W] b[1].  log_prob DEV f32 [units, elems] or
 * NULL; bits DEV f32 [units].  Built for (layers, width) = (3,3), (4,3), (3,5). */
int tfc_factorized_bits_forward(const void* y, const void* noise, void* y_hat, int dtype,
                                int64_t units, int64_t elems, int64_t channels, const float* params,
                                int layers, int width, float* log_prob, float* bits, void* stream);

/* Gradients of the above: gbits DEV f32 [units] = dL/dbits; dy DEV [units, elems] dtype =
 * dL/dy_hat through the likelihood (the caller adds the straight path); dparams DEV f32
 * [channels, P] is ADDED to (gradients w.r.t. the reparameterised values). */
int tfc_factorized_bits_backward(const void* y_hat, int dtype, int64_t units, int64_t elems,
                                 int64_t channels, const float* params, int layers, int width,
                                 const float* gbits, void* dy, float* dparams, void* stream);

/* The same with expected gradients — python/ops/math_ops.py:157-216, perturb_and_apply(expected_grads=True),
 * as continuous_batched.py:291-322 calls it when the entropy model was built with expected_grads=True:
 * dy = gbits * (log p(y + .5) - log p(y - .5)) / -ln 2 at the UNPERTURBED input y DEV [units, elems] dtype
 * (the expectation of the derivative over the uniform noise); dparams through log p(y_hat) as above. */
int tfc_factorized_bits_backward_expected(const void* y, const void* y_hat, int dtype, int64_t units,
                                          int64_t elems, int64_t channels, const float* params, int layers,
                                          int width, const float* gbits, void* dy, float* dparams, void* stream);

/* Training-time call of the indexed entropy model with a NoisyNormal prior, fused —
 * python/entropy_models/continuous_indexed.py:313-353 (`__call__(training=True)`: perturb_and_apply of
 * `_log_prob`), python/distributions/uniform_noise.py:117-156 over a Normal base:
 *   y_hat = y + noise (noise NULL: y itself);  log p = log(Phi((y_hat + .5) / scale) - Phi((y_hat - .5) / scale));
 *   bits[unit] = -sum log p / ln 2.
 * y, noise, y_hat DEV [units, elems] dtype (0 f32, 1 bf16); scale DEV f32 [units, elems] (> 0; the location is
 * the caller's: it shifts y); bits DEV f32 [units]. */
int tfc_noisy_normal_bits_forward(const void* y, const void* noise, const float* scale, void* y_hat, int dtype,
                                  int64_t units, int64_t elems, float* bits, void* stream);

/* Gradients of the above: dy DEV [units, elems] dtype = dL/dy_hat through the likelihood (the caller adds the
 * straight path), dscale DEV f32 [units, elems] = dL/dscale (overwritten).  y_in non-NULL selects expected
 * gradients (math_ops.py:157-216): dy = gbits * (log p(y_in + .5) - log p(y_in - .5)) / -ln 2 at the
 * unperturbed input. */
int tfc_noisy_normal_bits_backward(const void* y_in, const void* y_hat, const float* scale, int dtype,
                                   int64_t units, int64_t elems, const float* gbits, void* dy, float* dscale,
                                   void* stream);

/* The four calls above with the Laplace-mixture tail the entropy models take as `laplace_tail_mass`
 * (python/entropy_models/continuous_base.py:298-334, `_log_prob`): with m = laplace_tail_mass in (0, 1) and
 * Q = NoisyLaplace(0, 1),
 *   probs = (1 - m) p(y_hat) + m Q(y_hat);   log p := probs < 1e-10 ? log m + log Q(y_hat) : log probs,
 * in the likelihood, in its gradients (only the branch the reference's tf.where selects carries one) and in the
 * finite difference of expected gradients.  Q is evaluated in closed form (csrc/laplace_tail.h): the
 * reference's float32 difference of Laplace cumulatives loses all its digits beyond |y_hat| ~ 15, exactly where
 * this branch matters.  The backward calls take the unperturbed input y (y_in) or NULL like
 * tfc_noisy_normal_bits_backward: non-NULL selects expected gradients.  The Laplace component sits at 0: the
 * NoisyNormal calls are for a prior whose location the caller has subtracted from y. */
int tfc_factorized_bits_forward_tail(const void* y, const void* noise, void* y_hat, int dtype, int64_t units,
                                     int64_t elems, int64_t channels, const float* params, int layers, int width,
                                     float laplace_tail_mass, float* log_prob, float* bits, void* stream);
int tfc_factorized_bits_backward_tail(const void* y, const void* y_hat, int dtype, int64_t units, int64_t elems,
                                      int64_t channels, const float* params, int layers, int width,
                                      float laplace_tail_mass, const float* gbits, void* dy, float* dparams,
                                      void* stream);
int tfc_noisy_normal_bits_forward_tail(const void* y, const void* noise, const float* scale, void* y_hat, int dtype,
                                       int64_t units, int64_t elems, float laplace_tail_mass, float* bits,
                                       void* stream);
int tfc_noisy_normal_bits_backward_tail(const void* y_in, const void* y_hat, const float* scale, int dtype,
                                        int64_t units, int64_t elems, float laplace_tail_mass, const float* gbits,
                                        void* dy, float* dscale, void* stream);

/* ------------------------------------------------------------------------ */
/* HiFiC discriminator and GAN loss                                         */
/* ------------------------------------------------------------------------ */

/* Spectral normalisation of a convolution kernel — models/hific/archs.py:340-367 (`arch_ops.conv2d(..., use_sn=True)`
 * of compare_gan, which the reference imports at archs.py:24), one power iteration, epsilon 1e-12:
 *   W = kernel [kh, kw, cin, cout] read as [rows = kh kw cin, cols = cout];  l2n(a) = a rsqrt(max(sum a^2, 1e-12))
 *   v = l2n(W^T u);   u' = l2n(W v);   sigma = u'^T W v;   w_sn = W / sigma  (the same layout as W).
 * w, u [rows], w_sn, u_out [rows], v_out [cols], sigma [1]: DEV float32.  No float atomics: two calls, equal bits. */
int tfc_spectral_norm_forward(const float* w, const float* u, int64_t rows, int64_t cols, float* w_sn, float* u_out,
                              float* v_out, float* sigma, void* stream);
/* Its backward (the reference relies on TF autodiff with u' and v held constant): g = dL/dw_sn,
 *   dw = g / sigma - (<g, W> / sigma^2) u' v^T.      u = u' and v, sigma as the forward wrote them. */
int tfc_spectral_norm_backward(const float* g, const float* w, const float* u, const float* v, const float* sigma,
                               int64_t rows, int64_t cols, float* dw, void* stream);

/* The discriminator's front end — models/hific/archs.py:342-347 (lrelu, tf.image.resize NEAREST, tf.concat) plus the
 * zero channels the next convolution wants, one pass:
 *   out[n, y, x, :] = x[n, y, x, :image_channels] | lrelu(latent[n, sy, sx, :latent_channels]) | zeros
 *   sy = min(floor((2 y + 1) latent_height / (2 height)), latent_height - 1), sx likewise; lrelu(a) = max(a, 0.2 a).
 * x DEV [n, height, width, image_channels], latent DEV [n, latent_height, latent_width, latent_channels] (the latent
 * branch's convolution output), out DEV [n, height, width, padded_channels]; dtype 0 f32, 1 bf16.
 * image_channels + latent_channels <= 16 and <= padded_channels, a multiple of 4 up to 1024; axes up to 32768. */
int tfc_disc_front_forward(const void* x, const void* latent, void* out, int dtype, int64_t n, int64_t height,
                           int64_t width, int64_t latent_height, int64_t latent_width, int image_channels,
                           int latent_channels, int padded_channels, void* stream);
/* Its backward: g = dL/dout;  dx = g[..., :image_channels];  dlatent[n, sy, sx, c] = (latent > 0 ? 1 : 0.2) times the
 * sum of g[n, y, x, image_channels + c] over the pixels whose source is (sy, sx), in a fixed order. */
int tfc_disc_front_backward(const void* g, const void* latent, void* dx, void* dlatent, int dtype, int64_t n,
                            int64_t height, int64_t width, int64_t latent_height, int64_t latent_width,
                            int image_channels, int latent_channels, int padded_channels, void* stream);

/* arch_ops.lrelu(net, leak=0.2) — models/hific/archs.py:351, 358, 363 — in place: y = max(y, 0.2 y), `count` values. */
int tfc_lrelu_forward(void* y, int dtype, int64_t count, void* stream);
/* Its backward fused with the bias gradient of the convolution in front of it, one pass over gy and y [pixels,
 * channels]: gm = gy (y > 0 ? 1 : 0.2) (dtype), dbias[c] = sum over pixels of gm (float32, before gm is rounded; fixed
 * order).  masked = 0: no activation, only dbias = the sum of gy (y and gm unused).  dbias may be NULL. */
int tfc_lrelu_bias_backward(const void* gy, const void* y, void* gm, float* dbias, int dtype, int64_t pixels,
                            int64_t channels, int masked, void* stream);

/* compare_gan's non_saturating loss as models/hific/model.py:616-638 calls it.  logits DEV [2 half], real half first;
 * sce(x, z) = max(x, 0) - x z + log1p(exp(-|x|));
 *   out[0] = d_loss = mean sce(real, 1) + mean sce(fake, 0);   out[1] = g_loss = mean sce(fake, 1);
 *   out[2] = mean sigmoid(real);   out[3] = mean sigmoid(fake)   (model.py:761-762).   out DEV float32 [4]. */
int tfc_gan_loss_forward(const void* logits, int dtype, int64_t half, float* out, void* stream);
/* grad = *scale (sigmoid(x) - z) / half for mode 0 (d_loss) or, mode 1 (g_loss), the fake half with z = 1 and zeros for
 * the real half.  scale DEV float32 [1]: the incoming gradient of the loss.  grad DEV [2 half] dtype. */
int tfc_gan_loss_backward(const void* logits, const float* scale, int dtype, int64_t half, int mode, void* grad,
                          void* stream);

/* ------------------------------------------------------------------------ */
/* Entropy-constrained vector quantisation (the toy-source VECVQ model)     */
/* ------------------------------------------------------------------------ */

/* models/toy_sources/vecvq.py:53-71 with the distortion of compression_model.py:88-95, without the [N, K] cost matrix:
 *   dist[n, k] = s sum_d (x[n, d] - c[k, d])^2,  s = 1 (distortion 0, sse) or 1 / D (distortion 1, mse);
 *   index[n] = argmin_k (rates[k] + lmbda dist[n, k]), ties to the LOWEST k (as tf.argmin);
 *   rate[n] = rates[index[n]];  distortion[n] = dist[n, index[n]];  counts[k] = the number of rows with index k.
 * x DEV f32 [N, D], codebook DEV f32 [K, D], rates DEV f32 [K]; index DEV i32 [N], rate, distortion DEV f32 [N],
 * counts DEV i32 [K] or NULL.  The distance is always evaluated as the difference (x - c)^2.  index is in [0, K)
 * whatever the inputs (a NaN cost never wins).  D in [1, 2^20], K in [1, 2^24], N >= 0 (N == 0 launches nothing),
 * lmbda finite: checked on the host before anything is launched. */
int tfc_vecvq_assign(const float* x, const float* codebook, const float* rates, int64_t n, int64_t k, int64_t d,
                     float lmbda, int distortion, int* index, float* rate, float* dist, int* counts, void* stream);

/* Gradients of tfc_vecvq_assign (models/toy_sources/vecvq.py:65-71 differentiated; compression_model.py:88-95) for
 * g_rate = dL/drate, g_dist = dL/ddistortion, DEV f32 [N], either NULL meaning zero.  Each output is written only if
 * its pointer is not NULL:
 *   d_rates[k]       = sum_{n: index[n] = k} g_rate[n]
 *   d_codebook[k, :] = 2 s sum_{n: index[n] = k} g_dist[n] (c_k - x_n)      (the difference itself is accumulated)
 *   d_x[n, :]        = 2 s g_dist[n] (x_n - c_index[n])
 * Codewords nobody chose get exact zeros.  Deterministic: a gather with no float atomics; every sum runs in ascending n
 * within ranges fixed by (N, K, D), and the ranges are combined in ascending order.  A row whose index is outside
 * [0, K) contributes nothing. */
int tfc_vecvq_backward(const float* x, const float* codebook, const int* index, const float* g_rate,
                       const float* g_dist, int64_t n, int64_t k, int64_t d, int distortion, float* d_rates,
                       float* d_codebook, float* d_x, void* stream);

/* ------------------------------------------------------------------------ */
/* YUV4MPEG2 frames and YCbCr <-> RGB (python/datasets/y4m_dataset.py)      */
/* ------------------------------------------------------------------------ */

/* The de-interleaving of cc/kernels/y4m_dataset_kernels.cc:165-178 (one frame, one byte at a time, on the host) for
 * num_frames frames at once.  raw DEV u8 [raw_bytes]: frame n's planes Y [height, width], U and V [h, w] lie back to
 * back from byte first_offset + n frame_stride; chroma is 420 (h = height / 2, w = width / 2) or 444 (h = height,
 * w = width), as the header's C parameter reads.  y DEV u8 [num_frames, height, width, 1], cbcr DEV u8
 * [num_frames, h, w, 2] with cbcr[..., 0] = U and cbcr[..., 1] = V, both contiguous; cbcr 2-byte aligned, nothing else
 * need be aligned.  Only plane bytes are read.  Checked on the host before anything is launched: sizes positive (width,
 * height up to 2^20, num_frames height < 2^31), even width and height for 420, frame_stride >= the bytes of a frame,
 * first_offset >= 0, and first_offset + (num_frames - 1) frame_stride + frame bytes <= raw_bytes.  num_frames == 0
 * launches nothing. */
int tfc_y4m_unpack(const void* raw, int64_t raw_bytes, int64_t num_frames, int64_t width, int64_t height, int chroma,
                   int64_t frame_stride, int64_t first_offset, void* y, void* cbcr, void* stream);

/* The inverse, for writing frames (the reference has no writer): the planes of y and cbcr go to raw at the same
 * offsets.  Only plane bytes are written: what lies in front of first_offset, between frames (frame_stride beyond the
 * bytes of a frame) and behind the last frame is left as it is.  Arguments and checks as for tfc_y4m_unpack. */
int tfc_y4m_pack(const void* y, const void* cbcr, void* raw, int64_t raw_bytes, int64_t num_frames, int64_t width,
                 int64_t height, int chroma, int64_t frame_stride, int64_t first_offset, void* stream);

/* (y, cbcr) as tfc_y4m_unpack writes them -> rgb DEV [num_frames, height, width, 3] on the 0...255 scale, in one kernel.
 * The reference has no counterpart (its models are fed RGB PNGs).  With (Kr, Kb) = (0.299, 0.114) for matrix 0
 * (bt601) or (0.2126, 0.0722) for matrix 1 (bt709) and Kg = 1 - Kr - Kb:
 *   Y' = y, C' = c - 128 (full_range 1)  or  Y' = (y - 16) 255 / 219, C' = (c - 128) 255 / 224 (full_range 0);
 *   R = Y' + 2 (1 - Kr) Cr',  B = Y' + 2 (1 - Kb) Cb',  G = Y' - (2 Kr (1 - Kr) / Kg) Cr' - (2 Kb (1 - Kb) / Kg) Cb'
 * (the four coefficients in float64 on the host, float32 in the kernel).  420 chroma is upsampled first: upsample 0
 * (nearest) c[i / 2, j / 2]; upsample 1 (bilinear, centre siting, separable) row 2m takes 0.75 c[m] + 0.25 c[max(m - 1,
 * 0)], row 2m + 1 takes 0.75 c[m] + 0.25 c[min(m + 1, h - 1)], columns alike.  clip != 0 clamps to [0, 255].
 * dtype 0: uint8, always clamped, rounded half to even; 1: float32; 2: bfloat16 (round to nearest even).
 * Checked on the host: the sizes as for tfc_y4m_unpack, and the matrix, full_range, upsample and dtype codes. */
int tfc_ycbcr_to_rgb(const void* y, const void* cbcr, void* rgb, int64_t num_frames, int64_t width, int64_t height,
                     int chroma, int matrix, int full_range, int upsample, int dtype, int clip, void* stream);

/* The inverse (no counterpart in the reference): rgb DEV [num_frames, height, width, 3] of dtype (codes as above), 0...255
 * -> y, cbcr DEV u8 as above, in one kernel:
 *   Y' = Kr R + Kg G + Kb B,  Cb' = (B - Y') / (2 (1 - Kb)),  Cr' = (R - Y') / (2 (1 - Kr));
 * 420 chroma is the mean of each 2 x 2 block of Cb' / Cr'; then the range scaling is undone, the result clamped to
 * [0, 255] and rounded half to even.  The same host-side checks. */
int tfc_rgb_to_ycbcr(const void* rgb, int dtype, void* y, void* cbcr, int64_t num_frames, int64_t width,
                     int64_t height, int chroma, int matrix, int full_range, void* stream);

/* ------------------------------------------------------------------------ */
/* Training: random crops and the Keras Adam step (models/bls2017.py:198-270) */
/* ------------------------------------------------------------------------ */

/* num_patches random crops in one launch (tf.image.random_crop per image on host threads, bls2017.py:198-200).
 * pool DEV u8 [pool_bytes]: decoded images back to back, each [H_i, W_i, 3] row-major.  table DEV int64
 * [num_patches, 4], 8-byte aligned: per patch the byte offset of the image's first pixel in pool, the image width in
 * pixels, top and left.  out DEV [num_patches, patchsize, patchsize, 3], contiguous and 16-byte aligned, of dtype 0
 * (uint8), 1 (float32) or 2 (bfloat16): out[b, r, c, k] = pool[offset_b + ((top_b + r) W_b + left_b + c) 3 + k], the
 * integers 0...255, which all three types hold exactly.  Only the 3 patchsize bytes of each patch row are read, from
 * whatever address they have, so no byte outside [0, pool_bytes) is touched.  The table lives on the device and is
 * not read by the host: a row with a negative entry, a width, top or left above 2^24, or with
 * offset + ((top + patchsize - 1) W + left + patchsize) 3 > pool_bytes is not read from at all and yields zeros; callers
 * check their rows before the upload (ops/train_ops.py raises).  Checked on the host: patchsize in [1, 2^15], the dtype
 * code, num_patches patchsize^2 3 < 2^31, the pointers and their alignment.  num_patches == 0 launches nothing. */
int tfc_crop_patches(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t num_patches,
                     int64_t patchsize, int dtype, void* out, void* stream);

/* num_patches random crops of RESIZED images in one launch: HiFiC's training input (models/hific/model.py:316-351), where
 * tf.image.resize_images resizes every whole image on a host thread and tf.image.random_crop keeps one patch.  Here
 * only the patch's pixels are computed and the resized image never exists.  pool DEV u8 [pool_bytes] as for
 * tfc_crop_patches.  table DEV int64 [num_patches, 7], 8-byte aligned: per patch the byte offset of the image's first
 * pixel in pool, the image's width W and height H, the resized width OW and height OH, and top and left IN THE RESIZED
 * IMAGE.  out DEV [num_patches, patchsize, patchsize, 3], contiguous and 16-byte aligned, of dtype 1 (float32) or 2
 * (bfloat16); uint8 is not offered, the values are not integers.  The definition is TF1's resize_bilinear with
 * align_corners=False and half_pixel_centers=False (third-party code, not part of the reference tree).  For out[b, i, j, c]:
 *   sy = float32(H) / float32(OH)          sx = float32(W) / float32(OW)          (float32 division)
 *   py = float32(top + i) * sy             px = float32(left + j) * sx            (float32 product)
 *   y0 = min(floor(py), H - 1)   y1 = min(y0 + 1, H - 1)   wy = py - float32(y0)  (x0, x1, wx alike)
 *   t = tl + (tr - tl) * wx      b = bl + (br - bl) * wx   v = t + (b - t) * wy
 * with tl, tr, bl, br the bytes of channel c at (y0, x0), (y0, x1), (y1, x0), (y1, x1) as float32.  Every operation is
 * rounded to float32 on its own: no fused multiply-add.  bfloat16 is v rounded to nearest even.  Only bytes of the
 * image itself are read.  The table lives on the device and is not read by the host: a row with a negative entry, with
 * W, H, OW or OH outside [1, 2^24], with top + patchsize > OH or left + patchsize > OW, or with offset + 3 W H >
 * pool_bytes is not read from at all and yields zeros; callers check their rows before the upload (ops/train_ops.py
 * raises).  Checked on the host: patchsize in [1, 2^15], the dtype code, num_patches patchsize^2 3 < 2^31, the pointers
 * and their alignment.  num_patches == 0 launches nothing. */
int tfc_scale_crop_patches(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t num_patches,
                           int64_t patchsize, int dtype, void* out, void* stream);

/* One launch takes at most this many tensors; a workgroup takes one chunk of this many elements of one tensor. */
#define TFC_KERAS_ADAM_CAPACITY 64
#define TFC_KERAS_ADAM_CHUNK 4096

/* One optimiser step of tf.keras.optimizers.Adam (Keras 2.14 `update_step`; third-party code, not part of the
 * reference tree) over count <= TFC_KERAS_ADAM_CAPACITY float32 tensors in one launch.  params, grads, ms, vs and
 * numels are HOST arrays of count entries: DEV pointers (4-byte aligned; 16-byte aligned tensors take 16-byte
 * accesses) and element counts; numels[k] == 0 is legal.  Every element is updated in float32, in exactly this order
 * of individually rounded operations (no fused multiply-add; division and square root correctly rounded):
 *   m' = m + (g - m) * c1
 *   v' = v + (g * g - v) * c2
 *   p' = p - (m' * alpha) / (sqrt(v') + eps)
 * The caller passes c1 = float32(1 - beta_1), c2 = float32(1 - beta_2), eps = float32(epsilon) and
 * alpha = float32(lr sqrt(1 - beta_2^t) / (1 - beta_1^t)), computed in float64 and rounded once, t counting from 1.
 * So epsilon is added to sqrt(v'), not to the bias-corrected sqrt(v_hat), and both bias corrections sit in alpha.
 * skip: DEV int32, 4-byte aligned, or null.  When *skip != 0 the launch writes nothing at all: a non-finite loss stops
 * the update without a host round trip.  The table travels in the kernel arguments: nothing is uploaded or allocated.
 * Checked on the host: count, null pointers of non-empty tensors, alignment, non-negative element counts. */
int tfc_keras_adam(void* const* params, const void* const* grads, void* const* ms, void* const* vs,
                   const int64_t* numels, int count, float alpha, float c1, float c2, float eps, const int32_t* skip,
                   void* stream);

/* ------------------------------------------------------------------------ */
/* LVAC: inverse RAHT and the per-point decoder (models/lvac/lvac.ipynb)    */
/* ------------------------------------------------------------------------ */

/* Inverse RAHT down a binary tree of octree prefixes (the notebook's Model.synthesize without its repeat and
 * unsorted_segment_sum).  Level l turns rows[l] parent rows into child rows:
 *   child[c, :] = parent[child_parent[c], :] + child_weight[c] * ac[l][child_ac[c], :]     (child_ac < 0: no AC term)
 * dc DEV f32 [n_root, channels]; ac HOST array of `levels` DEV f32 pointers [AC rows of the level, channels] (ignored
 * for a level without AC rows); out DEV f32 [n_out, channels].  desc HOST and desc_dev DEV hold the same int64
 * [levels, 10]: child rows, parent rows, AC rows, then the offsets, in 4-byte words of `tables`, of child_parent (i32),
 * child_ac (i32), child_weight (f32), parent_first (i32), parent_count (i32), ac_left (i32), ac_coeff (f32).  tables DEV,
 * table_words words long.  Checked on the host before any launch: levels <= 64, channels in [1, 65536], every level's
 * children = parents + AC rows, the chain n_root -> ... -> n_out, every table inside the buffer.  The table VALUES are
 * the caller's (ops/lvac_ops.py RahtTree checks them once); whatever they hold, a kernel reads nothing outside the
 * tensors: an index out of range contributes zero.  A level without AC rows is the identity and launches nothing;
 * consecutive levels of at most 4096 elements share one single-workgroup launch.  Gathers only, no atomics:
 * bit-identical from call to call. */
int tfc_raht_forward(const float* dc, int64_t n_root, const float* const* ac, const int64_t* desc,
                     const int64_t* desc_dev, const int32_t* tables, int64_t table_words, int levels, int64_t channels,
                     float* out, int64_t n_out, void* stream);
/* Its gradients, from d_out DEV f32 [n_out, channels], level by level upwards:
 *   d_parent[i, :] = sum of d_child over the node's parent_count[i] (1 or 2) children from parent_first[i]
 *   d_ac[l][k, :]  = ac_coeff[k] * d_child[ac_left[k], :] + d_child[ac_left[k] + 1, :]
 * d_ac HOST array of `levels` DEV f32 pointers (written; ignored for a level without AC rows), d_dc DEV f32
 * [n_root, channels]. */
int tfc_raht_backward(const float* d_out, int64_t n_out, float* const* d_ac, const int64_t* desc,
                      const int64_t* desc_dev, const int32_t* tables, int64_t table_words, int levels,
                      int64_t channels, float* d_dc, int64_t n_root, void* stream);

/* The per-point decoder and its squared error (Model.reconstruct_at_level and evaluate_reconstruction_at_level with
 * the "mlp" extractor), without the [N, hidden] activations:
 *   recon[n, :] = A (W2^T relu(W1^T [position[n]; z[index[n]]] + b1) + b2) + o,   clipped to [0, 255] if clip
 *   sse         = sum_n sum_r (recon[n, r] - target[n, r])^2
 * z DEV f32 [n_blocks, channels]; index DEV i32 [n]; position DEV f32 [n, 3] or NULL (W1 then has `channels` rows,
 * else 3 + channels with the position rows first); w1 [rows, hidden], b1 [hidden], w2 [hidden, 3], b2 [3] DEV f32;
 * affine HOST f32 [12]: A row-major, then o; target DEV f32 [n, 3].  Outputs: recon DEV f32 [n, 3] or NULL; gerr DEV
 * f32 [n, 3] or NULL, recon - target where the gradient flows and 0 where the clip cut it (what the backward needs);
 * sse DEV f32 [1], per-workgroup partial sums added in a fixed order.  All float32 on the vector unit.  channels in
 * [1, 32], hidden in [1, 1024] (csrc/lvac_params.h), checked on the host.  An index outside [0, n_blocks) reads nothing
 * and stands for a zero latent.  n == 0 writes sse = 0. */
int tfc_point_mlp_forward(const float* z, const int32_t* index, const float* position, const float* w1,
                          const float* b1, const float* w2, const float* b2, const float* affine, const float* target,
                          int64_t n, int64_t n_blocks, int channels, int hidden, int clip, float* recon, float* gerr,
                          float* sse, void* stream);
/* Its gradients for g_sse = dL/dsse (DEV f32 [1]) and the gerr of the forward call.  d_params DEV f32
 * [rows hidden + hidden + 3 hidden + 3] or NULL: dW1, db1, dW2, db2 one after the other; d_z DEV f32
 * [n_blocks, channels] or NULL.  block_offset DEV int64 [n_blocks + 1]: the points of block b are
 * [block_offset[b], block_offset[b + 1]) (index non-decreasing).  The hidden activations are recomputed per tile of 128
 * points.  Deterministic, no atomics: parameter gradients are accumulated by at most 128 tile groups and merged in
 * ascending order; the latent gradient is written per point ([n, channels]) and summed per block in a fixed order. */
int tfc_point_mlp_backward(const float* z, const int32_t* index, const int64_t* block_offset, const float* position,
                           const float* w1, const float* b1, const float* w2, const float* b2, const float* affine,
                           const float* gerr, const float* g_sse, int64_t n, int64_t n_blocks, int channels,
                           int hidden, float* d_params, float* d_z, void* stream);

/* ------------------------------------------------------------------------ */
/* Scale-space warp (Agustsson et al., "Scale-space flow for end-to-end     */
/* optimized video compression", CVPR 2020, section 3.1)                    */
/* ------------------------------------------------------------------------ */

/* The definition is this project's own (the paper fixes the idea, not the taps, the borders or the clamps); parity with
 * the authors' trained models is unpinned.  All tensors DEV f32, contiguous, channels last, 16-byte aligned.
 *
 * The scale-space volume (section 3.1, "scale-space volume"): x [n, h, w, channels] -> volume
 * [n, num_levels + 1, h, w, channels].  Plane 0 is x.  Plane p >= 1 is x blurred separably, along W then along H, with
 * sigma_p = sigma0 2^(p - 1) and taps w_t = exp(-t^2 / (2 sigma_p^2)), |t| <= R_p = ceil(3 sigma_p).  Taps that fall
 * outside the image are dropped and the rest renormalised:
 *   out[i] = sum_t w_t x[i + t] / sum_t w_t,     both sums over the t with 0 <= i + t < n
 * so a constant image stays constant; the norm of a pixel is norm_row[j] norm_col[i].  No pyramid approximation.
 * Two launches: one row pass that reads each row segment once and writes plane 0 and all row-blurred planes, one column
 * pass with the plane as a grid dimension.  The taps and their running sums are computed here in double and travel in
 * the kernel arguments.  Checked on the host before any launch: channels in [1, 8], num_levels in [1, 8], sigma0 > 0,
 * sigma0 2^(num_levels - 1) <= 64, h and w in [1, 2^14], n (num_levels + 1) h w channels < 2^31, null pointers,
 * alignment.  n == 0 launches nothing.  The row-blurred planes (4 n num_levels h w channels bytes) come from the
 * library's block cache. */
int tfc_scale_space_volume(const float* x, float* volume, int64_t n, int64_t h, int64_t w, int channels,
                           int num_levels, double sigma0, void* stream);
/* Its adjoint: g_volume [n, num_levels + 1, h, w, channels] -> g_x [n, h, w, channels],
 *   g_x = g_volume[:, 0] + sum over p (ascending) of corr_W(corr_H(g_volume[:, p] / norm_p))
 * where corr is the same zero-padded symmetric correlation and norm_p[i, j] = norm_row[j] norm_col[i] of plane p: a
 * gather, no scatter, bit-identical from call to call.  The same checks. */
int tfc_scale_space_volume_backward(const float* g_volume, float* g_x, int64_t n, int64_t h, int64_t w, int channels,
                                    int num_levels, double sigma0, void* stream);
/* The warp (section 3.1, "scale-space warp"): flow [n, h, w, 3] = (dx along W in pixels, dy along H, s the plane
 * coordinate) samples the volume trilinearly.  For output pixel (i, j), with M = num_levels:
 *   px = fminf(fmaxf(float32(j) + dx, 0), w - 1)    py likewise with i, dy, h    pz = fminf(fmaxf(s, 0), M)
 *   x0 = min(floor(px), max(w - 2, 0))   x1 = min(x0 + 1, w - 1)   wx = px - x0      (y and z alike; z1 = min(z0 + 1, M))
 *   out[n, i, j, c] = sum over the 8 corners of (wz wy) wx volume[n, z, y, x, c]     (z outermost, x innermost)
 * fmaxf sends a NaN coordinate to 0; whatever flow holds, no address outside the volume is formed.  One launch, one
 * output pixel per lane, the channels of a corner loaded together, 16-byte accesses when channels is 4 or 8. */
int tfc_scale_space_warp_forward(const float* volume, const float* flow, float* out, int64_t n, int64_t h, int64_t w,
                                 int channels, int num_levels, void* stream);
/* The warp's gradients for g [n, h, w, channels]; each output may be NULL.
 *   g_flow [n, h, w, 3]: a gather per output pixel (needs `volume`).  d out / d dx is the x-derivative of the trilinear
 *     form (differences of corners, weighted by the other two axes) where 0 < float32(j) + dx < w - 1 strictly, and 0
 *     where the coordinate was clamped or is NaN; dy and s alike (0 < s < M).  Channels are summed in ascending order.
 *   g_volume [n, M + 1, h, w, channels]: d out / d volume is the corner weights.  The scatter of g weight accumulates
 *     in 64-bit integers with vector global atomics; integer addition is associative, so the sums do not depend on the
 *     arrival order.  A two-stage, fixed-order device reduction yields gmax = max |g| (NaN if any g is not finite); with
 *     e = floor(log2 gmax) + 1 a contribution is llrint(double(g weight) 2^(40 - e)) and the gradient is
 *     float32(double(sum) 2^(e - 40)).  gmax == 0 gives all-zero gradients without a scatter; a non-finite gmax fills
 *     g_flow, g_volume and g_x with NaN.  Nothing is read back to the host.
 *   g_x [n, h, w, channels]: tfc_scale_space_volume_backward (with sigma0, otherwise unused) applied to the integer
 *     planes directly; the float volume gradient is not formed unless g_volume is asked for as well.
 * The scatter requires h w <= 2^22 (then a sum of h w contributions below 2^40 fits 63 bits), checked on the host like
 * the rest.  The integer planes (tfc_scale_space_workspace bytes) come from the library's block cache and are zeroed
 * in stream order. */
int tfc_scale_space_warp_backward(const float* g, const float* volume, const float* flow, float* g_flow,
                                  float* g_volume, float* g_x, double sigma0, int64_t n, int64_t h, int64_t w,
                                  int channels, int num_levels, void* stream);
/* The bytes of the backward's integer planes, 8 n (num_levels + 1) h w channels; -1 (and tfc_last_error) when the
 * shape fails the checks above. */
int64_t tfc_scale_space_workspace(int64_t n, int64_t h, int64_t w, int channels, int num_levels);

/* ------------------------------------------------------------------------ */
/* Spatial context model (Minnen, Ballé, Toderici 2018)                     */
/* ------------------------------------------------------------------------ */

/* The autoregressive half of "Joint autoregressive and hierarchical priors for learned image compression" (NeurIPS
 * 2018, section 2 and figure 2): the reference tree publishes that model's rate-distortion curves
 * (results/image_compression) and lists its context-free variant (models/tfci.py, `mbt2018-mean`) but carries no
 * program text for the context model, so the definition is this project's own.  With y [batch, Hl, Wl, M] the latent,
 * psi [batch, Hl, Wl, P] the hyper-synthesis output, y_hat = 0 outside the latent, and positions taken in any order
 * that puts (i - 2 .. i, all j) above and (i, < j) to the left first:
 *   ctx[i, j]  = bc + sum over the 12 causal taps (di < 0, or di == 0 and dj < 0; |di|, |dj| <= 2)
 *                of y_hat[i + di, j + dj] . Wc[di + 2, dj + 2]                                   M -> 2M
 *   h1 = lrelu(b1 + [ctx, psi] W1)   h2 = lrelu(b2 + h1 W2)   out = b3 + h2 W3                   lrelu slope 0.2
 *   mu = out[:M]     index_float = out[M:]     idx = tfc_index_prepare(index_float, num_scales)
 *   sym = int32(rint(y - mu))  (half to even)        y_hat = float32(sym) + mu
 * all float32.  Each dot product is summed in four partial sums (k mod 4, k ascending inside a tap, taps in
 * row-major order) combined as (s0 + s1) + (s2 + s3) and added to the bias; both entry points run the same device
 * function, so the decoder's y_hat equals the encoder's bit for bit on the same build and device kind.
 * `packed` DEV float32 [packed_floats], 16-byte aligned: the weights in the layout of csrc/context_params.h
 * (ctx_layout; the mask already applied).  `workspace` DEV, 16-byte aligned, tfc_context_workspace bytes.
 * Checked on the host before any launch: sizes (M, P, H1, H2 in [1, 65536] and one position's activations within
 * 60 KiB of LDS), Hl, Wl in [1, 2^24], batch Hl Wl <= 2^40, num_scales, packed_floats, null pointers, alignment.
 * batch == 0 launches nothing. */

/* Bytes of the workspace of the two calls below (the hyperprior half of the first layer for every position and one
 * decoder state per row); -1 (and tfc_last_error) when the sizes fail the checks.  Replaces nothing: TensorFlow's
 * allocator owns an op's scratch memory. */
int64_t tfc_context_workspace(int64_t batch, int64_t hl, int64_t wl, int m, int p, int h1, int h2);
/* The encoder side and the evaluation: every output is [batch, Hl, Wl, M].  ONE launch, one workgroup per image;
 * position (i, j) is of wavefront step j + 3 i, a step's positions go through the network together.  Replaces a host
 * loop over the Hl Wl positions of a masked convolution (python/layers/signal_conv.py:663-690 with a masked kernel),
 * three 1x1 convolutions and tf.round per position. */
int tfc_context_scan(const float* y, const float* psi, const float* packed, int64_t packed_floats, int64_t batch,
                     int64_t hl, int64_t wl, int m, int p, int h1, int h2, int num_scales, void* workspace,
                     int32_t* sym, int32_t* idx, float* mu, float* index_float, float* y_hat, void* stream);
/* The decoder side: blob / offsets DEV describe batch * Hl strings as tfc_decoder_create takes them with
 * src_on_device = 1 (row i of image b is string b * Hl + i, coded in raster order along the row, channels
 * innermost: what tfc_encoder_encode_quantized_indexed writes for [batch, Hl] streams of Wl * M elements, escapes
 * included); cdf_offset DEV int32 [num_scales].  y_hat = float32(symbol + cdf_offset[idx]) + mu.  ok DEV uint8
 * [batch * Hl]: EntropyDecodeFinalize's check per string (tfc_decoder_finalize_device).  ONE launch: the network and
 * the range decoder alternate inside it.  Replaces a host loop of the same network and one EntropyDecodeIndex call
 * (cc/kernels/range_coder_kernels.cc:360-429) per position.  Damaged strings end the call like intact ones (reads
 * past a string's end yield zeros, an escape's unary part is bounded) and show in `ok`. */
int tfc_context_decode(const tfc_tables* tables, const uint8_t* blob, const int64_t* offsets, const float* psi,
                       const float* packed, int64_t packed_floats, const int32_t* cdf_offset, int64_t batch,
                       int64_t hl, int64_t wl, int m, int p, int h1, int h2, int num_scales, void* workspace,
                       float* y_hat, uint8_t* ok, void* stream);

/* ------------------------------------------------------------------------ */
/* Checkerboard context model (He, Zheng, Sun, Wang, Qin 2021)              */
/* ------------------------------------------------------------------------ */

/* The two-pass context model of "Checkerboard context model for efficient learned image compression" (CVPR 2021).
 * The reference tree carries no program text for it: the definition, the stream format and the layer shapes are this
 * project's own, and parity with anyone's checkpoints is unpinned.  With y [batch, Hl, Wl, M] the latent, psi [batch,
 * Hl, Wl, P] the hyper-synthesis output and y_hat = 0 outside the latent, position (i, j) is an ANCHOR when i + j is
 * even; pass 0 is the anchors, pass 1 the rest:
 *   taps       = (di, dj) in [-2, 2]^2 with di + dj odd, row-major: 12 taps (every such neighbour of a pass-1
 *                position is an anchor)
 *   ctx[i, j]  = bc                                                            pass 0
 *              = bc + sum over the taps of y_hat[i + di, j + dj] . Wc[di + 2, dj + 2]     pass 1           M -> 2M
 *   h1 = lrelu(b1 + [ctx, psi] W1)   h2 = lrelu(b2 + h1 W2)   out = b3 + h2 W3                 lrelu slope 0.2
 *   mu = out[:M]     index_float = out[M:]     idx = tfc_index_prepare(index_float, num_scales)
 *   sym = int32(rint(y - mu))  (half to even)        y_hat = float32(sym) + mu
 * all float32.  COMPACT ORDER: the positions of one pass in raster order, channels innermost, [batch, N_p, M] with
 * N_0 = ceil(Hl Wl / 2), N_1 = floor(Hl Wl / 2); the slot of (i, j) is (i Wl + j) >> 1 when Wl is odd and
 * i (Wl / 2) + (j >> 1) when Wl is even.
 * Every output element is one chain of float32 fused multiply-adds that starts from its bias and takes the inputs in
 * ascending k (taps in row-major order and a tap's channels ascending; a neighbour outside the latent enters as
 * zeros; the 2M context features before the P hyperprior features): the order depends on (M, P, H1, H2) alone, not on
 * the batch, the tile of 32 positions a position falls in or its place there, so an image coded in a batch decodes
 * alone, bit for bit, on the same build and device kind.
 * `packed` DEV float32 [packed_floats]: the layout of csrc/context_params.h (ctx_layout), whose 12 x Mp rows of wc
 * hold these taps in row-major order (tap k is element 2 k + 1 of the 5x5 window).
 * Checked on the host before any launch: pass, sizes (as tfc_context_scan, and the activations of 32 positions within
 * 160 KiB of LDS, which the kernel declares in full), Hl, Wl, batch, num_scales, packed_floats, null pointers.
 * batch == 0, or a pass without positions (pass 1 of a 1x1 latent), launches nothing.
 * The two entries are tfc_scctx_params and tfc_scctx_place below with one group that is the whole latent, c_g = 0 and
 * M_g = M: the same kernels, the same checks (an error names the entry that was called and lists c_g and M_g too),
 * the same packed buffer. */

/* The parameters of one pass for all its positions, ONE launch (a workgroup per 32 positions of an image).  y_hat
 * DEV [batch, Hl, Wl, M] is read at the anchors (pass 1) and, when `y` is given, written at the pass's positions.
 * mu, index_float DEV float32 and idx DEV int32 [batch, N_pass, M] in compact order.  `y` DEV [batch, Hl, Wl, M] or
 * NULL (the decoder): when given, sym DEV int32 [batch, N_pass, M] is written as well.  Replaces a masked convolution
 * (python/layers/signal_conv.py:663-690 with a masked kernel), three 1x1 convolutions, tf.round and two gathers. */
int tfc_checkerboard_params(int pass, const float* y, float* y_hat, const float* psi, const float* packed,
                            int64_t packed_floats, int64_t batch, int64_t hl, int64_t wl, int m, int p, int h1, int h2,
                            int num_scales, float* mu, float* index_float, int32_t* idx, int32_t* sym, void* stream);
/* The decoder's store of a decoded pass: y_hat[position] = sym + mu, the same single float32 add, from compact sym
 * (float32, as the entropy model's decoder returns it) and mu [batch, N_pass, M] into y_hat [batch, Hl, Wl, M]. */
int tfc_checkerboard_place(int pass, const float* sym, const float* mu, float* y_hat, int64_t batch, int64_t hl,
                           int64_t wl, int m, void* stream);

/* ------------------------------------------------------------------------ */
/* Space-channel context model, SCCTX (after He, Yang, Peng, Mao, Qin, Wang 2022) */
/* ------------------------------------------------------------------------ */

/* The context model of "ELIC: efficient learned image compression with unevenly grouped space-channel contextual
 * adaptive coding" (CVPR 2022): the channels of the latent are cut into G groups, the checkerboard above runs inside
 * every group, and a group sees all earlier groups.  The reference tree carries no program text for it: the
 * definition, the stream format and the layer shapes are this project's own, and parity with anyone's checkpoints is
 * unpinned.  With y [batch, Hl, Wl, M], psi [batch, Hl, Wl, P], y_hat = 0 outside the latent, groups (M_0 .. M_{G-1})
 * with sum M and c_g = M_0 + .. + M_{g-1}, the coding order is group 0 pass 0, group 0 pass 1, group 1 pass 0, ...:
 * 2 G steps, each parallel over the positions of its pass (anchors, i + j even, are pass 0).  Step (g, pass):
 *   ctx_g = bc_g
 *         + sum over ALL 25 taps (di, dj) of the 5x5 window, row-major, channels c < c_g ascending, of
 *               y_hat[i + di, j + dj, c] . Wch_g[di + 2, dj + 2, c, :]                       (nothing for g = 0)
 *         + pass 1 only: sum over the 12 checkerboard taps (di + dj odd, row-major), the group's channels ascending, of
 *               y_hat[i + di, j + dj, c_g + c] . Wsp_g[di + 2, dj + 2, c, :]                              -> 2 M_g
 *   h1 = lrelu(b1_g + [ctx_g, psi] W1_g)   h2 = lrelu(b2_g + h1 W2_g)   out = b3_g + h2 W3_g        lrelu slope 0.2
 *   mu = out[:M_g]   index_float = out[M_g:]   idx = tfc_index_prepare(index_float, num_scales)
 *   sym = int32(rint(y[.., c_g + c] - mu))  (half to even)        y_hat[.., c_g + c] = float32(sym) + mu
 * all float32; compact order as above, [batch, N_pass, M_g].  With G = 1 this is the checkerboard model, term for
 * term and in the same order.
 * Every output element is one chain of float32 fused multiply-adds that starts from its bias and takes one input row
 * per fmaf in ascending k, in the order written above: the earlier-group taps, then the own-group taps, then (first
 * layer) the 2 M_g context rows, then the P hyperprior rows.  A neighbour outside the latent and a padded row enter
 * as zeros and are never skipped; K is never split across waves.  The order depends on (c_g, M_g, P, H1, H2) alone.
 * `packed` DEV float32 [packed_floats]: ONE GROUP's buffer in the layout of csrc/space_channel_params.h
 * (scctx_layout): ctx_layout(M_g, P, H1, H2) with Wsp_g on the checkerboard taps, then Wch_g [25][c_g padded][2 M_g].
 * Checked on the host before any launch: pass, M, c_g, M_g (the group inside the latent), the sizes (as
 * tfc_checkerboard_params with M_g for M: the activations of 32 positions of THIS group within 160 KiB of LDS), Hl,
 * Wl, batch, num_scales, packed_floats, null pointers.  batch == 0, or a pass without positions, launches nothing. */

/* The parameters of step (g, pass) for all its positions, ONE launch.  y_hat DEV [batch, Hl, Wl, M] is read at the
 * channels below c_g everywhere and (pass 1) at the group's channels at anchors; when `y` is given it is written at
 * the group's channels at the pass's positions.  mu, index_float DEV float32 and idx DEV int32 [batch, N_pass, M_g];
 * `y` DEV [batch, Hl, Wl, M] or NULL (the decoder): when given, sym DEV int32 [batch, N_pass, M_g] is written too. */
int tfc_scctx_params(int pass, const float* y, float* y_hat, const float* psi, const float* packed,
                     int64_t packed_floats, int64_t batch, int64_t hl, int64_t wl, int m, int cg, int mg, int p, int h1,
                     int h2, int num_scales, float* mu, float* index_float, int32_t* idx, int32_t* sym, void* stream);
/* The decoder's store of a decoded step: y_hat[position, c_g + c] = sym + mu, the same single float32 add, from
 * compact sym (float32) and mu [batch, N_pass, M_g] into y_hat [batch, Hl, Wl, M]. */
int tfc_scctx_place(int pass, const float* sym, const float* mu, float* y_hat, int64_t batch, int64_t hl, int64_t wl,
                    int m, int cg, int mg, void* stream);

/* Shifted-window attention (the attention of a Swin block; "Transformer-based Transform Coding", Zhu, Yang and Cohen,
 * ICLR 2022).  The definition is this library's own; parity with anyone's checkpoints is not pinned.
 *   qkv DEV [batch, height, width, 3 C] dtype (0 f32, 1 bf16), C = heads * head_dim; channel which * C + head *
 *   head_dim + j holds q (which = 0), k (1), v (2).  table DEV float32 [heads, (2 ws - 1)^2].  out DEV [batch, height,
 *   width, C] dtype, channel head * head_dim + j.  ws = window, s = shift (0 or ws / 2).
 * Padded grid: Hp = ceil(height / ws) ws, Wp likewise.  Window (wy, wx), token (ty, tx) sits at rolled coordinate
 * r = (wy ws + ty, wx ws + tx); its source coordinate is (yp, xp) = ((r_y + s) mod Hp, (r_x + s) mod Wp); it is VALID
 * iff yp < height and xp < width; its wrap flags are (r_y + s >= Hp, r_x + s >= Wp).
 * Per head, for a valid query i and the keys j of the same window:
 *   S_ij = head_dim^-1/2 q_i . k_j + table[head, (ty_i - ty_j + ws - 1) (2 ws - 1) + (tx_i - tx_j + ws - 1)]
 * j takes part iff it is valid and has the same two wrap flags as i; every other j has weight exactly 0 (it is
 * excluded, not given a large negative score).  P_i = softmax over the j that take part; out_i = sum_j P_ij v_j,
 * written at (yp, xp).  Invalid positions are neither read nor written; no padded, rolled or partitioned tensor is
 * made.  The definition is applied literally when Hp == ws too.
 * float32: products as float32 fmaf chains, softmax in float32.  bf16: both products on the bf16 MFMA with float32
 * accumulation, softmax in float32, exp(S - max) rounded to bf16 before P.V, the row sum from the unrounded values, out
 * rounded once.  A window's output depends on that window's tokens and the table only: it is bit-identical whatever
 * else is in the image or the batch.
 * window in {4, 8}, head_dim in {16, 32}, heads >= 1, batch, height, width >= 1; qkv and out 16-byte aligned. */
int tfc_window_attention_forward(const void* qkv, const float* table, void* out, int dtype, int64_t batch,
                                 int64_t height, int64_t width, int heads, int head_dim, int window, int shift,
                                 void* stream);
/* Its backward, deterministic, S and P recomputed from qkv.  dout = dL/dout DEV [batch, height, width, C] dtype.  With
 * dP = dout V^T and dS = P o (dP - rowsum(dP o P)):
 *   dV = P^T dout,   dQ = head_dim^-1/2 dS K,   dK = head_dim^-1/2 dS^T Q      -> dqkv DEV [batch, height, width, 3 C] dtype
 *   dtable[head, rel] = sum over batches, windows and pairs of dS              -> dtable DEV float32, as table
 * dtable is summed through per-workgroup partials merged in a fixed order (no float atomics): two calls give the same
 * bits.  dqkv or dtable may be NULL: that gradient is not computed. */
int tfc_window_attention_backward(const void* qkv, const float* table, const void* dout, void* dqkv, float* dtable,
                                  int dtype, int64_t batch, int64_t height, int64_t width, int heads, int head_dim,
                                  int window, int shift, void* stream);

/* Layer normalisation over the last axis, on the ChannelNorm kernels (csrc/channel_norm.hip) with the BIASED variance:
 *   mean_p = sum_c x[p,c] / C;   var_p = sum_c (x[p,c] - mean_p)^2 / C
 *   y[p,c] = (x[p,c] - mean_p) * rsqrt(var_p + epsilon) * gamma[c] + beta[c];   residual != NULL: y += residual[p,c].
 * Arguments as tfc_channel_norm_forward (no ReLU); channels >= 1. */
int tfc_layer_norm_forward(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                           int dtype, int64_t pixels, int64_t channels, float epsilon, void* stream);
/* Its backward without the residual (whose gradient is g itself), xhat = (x - mean) rstd:
 *   dx = rstd (g gamma - sum_c(g gamma) / C - xhat sum_c(g gamma xhat) / C);  dgamma[c] = sum_p g xhat;  dbeta[c] = sum_p g
 * dgamma, dbeta DEV float32 [channels] or NULL, summed in a fixed order as tfc_channel_norm_backward does. */
int tfc_layer_norm_backward(const void* x, const void* g, const float* gamma, const float* beta, void* dx,
                            float* dgamma, float* dbeta, int dtype, int64_t pixels, int64_t channels, float epsilon,
                            void* stream);

/* Exact GELU, y = 0.5 x (1 + erf(x / sqrt 2)), `count` values of dtype (0 f32, 1 bf16), computed in float32. */
int tfc_gelu_forward(const void* x, void* y, int dtype, int64_t count, void* stream);
/* Its backward: dx = g (0.5 (1 + erf(x / sqrt 2)) + x exp(-x^2 / 2) / sqrt(2 pi)). */
int tfc_gelu_backward(const void* x, const void* g, void* dx, int dtype, int64_t count, void* stream);

/* The integer convolution layer of an integer network ("Integer Networks for Data Compression with Latent-Variable
 * Models", Balle, Johnston and Minnen, ICLR 2019, sections 2-3).  The definition is this library's own; parity with
 * anyone's checkpoints is not pinned.  NHWC; the geometry is exactly tfc_conv2d_down's (up = 0: zero padding (k / 2,
 * (k - 1) / 2), out = ceil(in / stride)) or tfc_conv2d_up's (up = 1: y[q s + phi] = sum_i x[i] w[phi + (q - i) s +
 * k / 2], out = in * stride), zeros outside the image, stride 1 or 2, any kh x kw from 1 to 9.
 *   v[n,p,o] = bias[o] + sum over taps t and i < cin of W[t,i,o] * x[n, src(p,t), i]        (exact, in int32)
 *   y[n,p,o] = min(max(floor((v + floor(c[o] / 2)) / c[o]), 0), out_max)                   (stored as uint8)
 * Both clamps are at or above 0: a negative v gives 0 and the division is only ever one of non-negative integers.
 *   x DEV [n, h, wd, cin]: int8 -128 ... 127 (x_unsigned = 0) or uint8 0 ... 255 (x_unsigned = 1)
 *   w DEV int8 [kh, kw, cout, cin] -128 ... 127: the layer's HWIO kernel with its last two axes swapped, so that the
 *     cin bytes of one (tap, output channel) are contiguous
 *   bias DEV int32 [cout], |bias| <= 2^29;  divisor DEV int32 [cout], 1 <= c <= 2^24 (the caller's duty: the values
 *     are not read on the host);  out_max 1 ... 255;  y DEV uint8 [n, oh, ow, cout], WRITTEN
 * cin must be a multiple of 32 and kh * kw * cin at most 32768: then 32768 * 128 * 255 < 2^30 and no intermediate
 * leaves int32, in any order of summation: the result is the same bytes on every device, build and tiling.  The kernel
 * (csrc/integer_conv.hip) sums on v_mfma_i32_16x16x64_i8, carries uint8 activations as a - 128 (zeros outside the
 * image included) with 128 * sum(W) added back, and divides with the exact unsigned division.  Every scalar argument
 * is checked on the host before the device is touched.  x and w 16-byte aligned; y 4-byte aligned where cout % 4 == 0. */
int tfc_integer_conv2d(const void* x, int x_unsigned, const int8_t* w, const int32_t* bias, const int32_t* divisor,
                       uint8_t* y, int64_t n, int64_t h, int64_t wd, int64_t cin, int64_t cout, int kh, int kw,
                       int stride, int up, int out_max, void* stream);

/* ------------------------------------------------------------------------ */
/* Gaussian-mixture entropy model: CDFs evaluated where they are coded      */
/* ------------------------------------------------------------------------ */
/* The discretized Gaussian mixture likelihood of "Learned Image Compression with Discretized Gaussian Mixture
 * Likelihoods and Attention Modules" (Cheng, Sun, Takeuchi, Katto, CVPR 2020): every element has K weights (as
 * logits), K means and K scales, K in [1, 4].  No table set spans that, so these entries take the parameters
 * themselves.  The definition (csrc/mixture_cdf.h) is this library's own; parity with anyone's
 * checkpoints is not pinned.  Symbols are rint(y) (no mean is subtracted), coded inside a window [lo, lo + L - 1],
 * 1 <= L <= 4096, |lo| <= 2^22, at precision 16:
 *   c_0 = 0,  c_L = 65536,  c_b = 2 b + floor(F(lo + b - 1/2) (65536 - 2 L)),  F(t) = sum_k softmax(logits)_k
 *   Phi((t - loc_k) / scale_k), F in float32 in one fixed operation order and clamped to [0, 1].
 * The parameters are DEV float32 PLANES [K][n]: plane k holds component k of every element.  scale > 0 and finite is
 * the caller's duty; any such value is safe.  One call takes at most 2^23 streams (or strings).  Strings decode on the
 * build and device kind that encoded them. */

/* The table the coder uses, dumped: cdf DEV int32 [n, L + 1].  Replaces a host-built table per element (the
 * reference has none: its conditional models index a fixed table set, python/entropy_models/continuous_indexed.py). */
int tfc_mixture_cdf(const float* logits, const float* loc, const float* scale, int k, int64_t n, int lo, int len,
                    int32_t* cdf, void* stream);

/* Bytes of the `blob` tfc_mixture_encode needs (every stream's worst case); -1 and tfc_last_error on bad sizes. */
int64_t tfc_mixture_blob_capacity(int64_t batch, int64_t elems, int64_t stream_symbols);

/* sym DEV int32 [batch, elems] (absolute symbols; one outside its entry's window is coded as the nearest end), cut
 * into ceil(elems / stream_symbols) streams per batch entry, the last one shorter where it has to be; parameter
 * planes [K][batch * elems]; lo, len DEV int32 [batch].  One wave per stream.  Writes the strings back to back into
 * blob DEV (tfc_mixture_blob_capacity bytes) and offsets DEV int64 [streams + 1], as tfc_encoder_result describes the
 * batched encoders' output; *overflow DEV uint32 is 0 unless a stream outgrew its slab (an internal error).  Enqueues
 * only.  Stands in for RangeEncode over a per-element table (cc/kernels/range_coding_kernels.cc:60-379): the strings
 * are those of tfc_range_encode(sym - lo, tfc_mixture_cdf(...), 16), byte for byte. */
int tfc_mixture_encode(const int32_t* sym, const float* logits, const float* loc, const float* scale, int k,
                       int64_t batch, int64_t elems, int64_t stream_symbols, const int32_t* lo, const int32_t* len,
                       uint8_t* blob, int64_t* offsets, uint32_t* overflow, void* stream);

/* The inverse: string j (blob, offsets DEV int64 [nstrings + 1]) is stream stream_index[j] of the layout above
 * (stream_index DEV int32 [nstrings], or NULL when nstrings is the number of streams and string j is stream j), so a
 * subset of the streams, or the streams in another order, can be decoded (no stream twice: the caller's duty); the symbols of a decoded stream go to its
 * place in out DEV int32 [batch, elems], the rest of out is left alone.  ok DEV uint8 [nstrings]: RangeDecoder::
 * Finalize's verdict (cc/lib/range_coder.h:144-169), and 0 as well where the string ends before digits the decoder
 * consumed while no carry was pending, or stream_index[j] names no stream.  The decoder reads zeros behind the end of
 * a string and every symbol it writes is inside the window, whatever the bytes are.  Stands in for RangeDecode
 * (range_coding_kernels.cc:232-379) over a per-element table. */
int tfc_mixture_decode(const uint8_t* blob, const int64_t* offsets, const int32_t* stream_index, int64_t nstrings,
                       const float* logits, const float* loc, const float* scale, int k, int64_t batch, int64_t elems,
                       int64_t stream_symbols, const int32_t* lo, const int32_t* len, int32_t* out, uint8_t* ok,
                       void* stream);

/* The training-time likelihood of the same mixture, fused — python/distributions/uniform_noise.py:117-156
 * (UniformNoiseAdapter) over a MixtureSameFamily of normals, i.e. NoisyNormalMixture:
 *   y_hat = y + noise (noise NULL: y itself);  lp_k = log(Phi((y_hat + .5 - loc_k) / scale_k) - Phi((y_hat - .5 -
 *   loc_k) / scale_k));  log p = logsumexp_k(log_softmax(logits)_k + lp_k);  bits[unit] = -sum log p / ln 2,
 * summed in a fixed order.  y, noise, y_hat DEV [units, elems] dtype (0 f32, 1 bf16); parameter planes DEV f32
 * [K][units * elems]; bits DEV f32 [units].  No Laplace tail, no expected gradients. */
int tfc_mixture_bits_forward(const void* y, const void* noise, const float* logits, const float* loc,
                             const float* scale, int k, void* y_hat, int dtype, int64_t units, int64_t elems,
                             float* bits, void* stream);
/* Its gradients in one launch, through the responsibilities softmax_k(logits_k + lp_k): dy DEV [units, elems] dtype
 * (through the likelihood; the caller adds the straight path), dlogits, dloc, dscale DEV f32 planes [K][units * elems],
 * all overwritten. */
int tfc_mixture_bits_backward(const void* y_hat, const float* logits, const float* loc, const float* scale, int k,
                              int dtype, int64_t units, int64_t elems, const float* gbits, void* dy, float* dlogits,
                              float* dloc, float* dscale, void* stream);

/* ------------------------------------------------------------------------ */
/* Interleaved rANS: one stream, up to 64 coder states at once              */
/* ------------------------------------------------------------------------ */
/* A second, opt-in stream format next to the range coder (csrc/ans_core.h): `lanes` rANS states
 * (a power of two in [1, 64]) code `lanes` consecutive elements of one stream per step.  These calls play the role of
 * EntropyEncodeIndex / EntropyEncodeChannel + Finalize and their decoding counterparts
 * (cc/kernels/range_coder_kernels.cc:191-322,360-471): the same `lookup` tables (a tfc_tables), the same index and
 * channel modes, the same escape mapping of values outside a row with a negative header.  THE BYTES ARE NOT THE
 * REFERENCE'S: the format is this library's own, and `lanes` is part of it (the decoder has to be given the encoder's).
 * value DEV int32 [streams, elems], the row's offset already subtracted; index DEV int32 [streams, elems], or NULL for
 * channel mode (element j of a stream takes row j mod rows).  One wave per stream; one call takes at most 2^23
 * streams of at most 2^27 elements.  Bad scalar arguments are refused on the host before anything is launched. */

/* Bytes of the `blob` tfc_ans_encode needs: per stream 4 words per element (4 calls of one word each) and the
 * states; -1 and tfc_last_error on bad sizes. */
int64_t tfc_ans_blob_capacity(int64_t streams, int64_t elems, int lanes);

/* Writes the strings back to back into blob DEV (tfc_ans_blob_capacity bytes) and offsets DEV int64 [streams + 1];
 * *overflow DEV uint32 is 0 unless a stream outgrew its slab (an internal error); status DEV int32 [streams] is 0, or
 * has bit 0 set where a value lay outside a row without escape (or on a symbol of zero width) and bit 1 where an index
 * named no row: that stream's string is not to be used.  Enqueues only, nothing is read back. */
int tfc_ans_encode(const tfc_tables* tables, const int32_t* index, const int32_t* value, int64_t streams,
                   int64_t elems, int lanes, uint8_t* blob, int64_t* offsets, uint32_t* overflow, int32_t* status,
                   void* stream);

/* The inverse: string j (blob, offsets DEV int64 [nstrings + 1]) is stream stream_index[j] (DEV int32 [nstrings], or
 * NULL when nstrings == streams and string j is stream j; no stream twice: the caller's duty).  A decoded stream's
 * values go to its row of out DEV int32 [streams, elems]; the rest of out is left alone.  ok DEV uint8 [nstrings] is 1
 * only where the string has its states and an even rest, every word was consumed and none was missing, and every
 * state ended at 2^16; 0 as well where stream_index[j] names no stream (nothing else is written then).  Words behind
 * the end of a string read as zero, a symbol search cannot leave its row: whatever the bytes are, nothing outside the
 * stream's own outputs is written. */
int tfc_ans_decode(const tfc_tables* tables, const uint8_t* blob, const int64_t* offsets, const int32_t* stream_index,
                   int64_t nstrings, const int32_t* index, int64_t streams, int64_t elems, int lanes, int32_t* out,
                   uint8_t* ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TFC_HIP_H_ */

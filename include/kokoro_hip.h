/* kokoro_hip.h -- C ABI of the MI355X-native Kokoro-82M acoustic path (libkokoro_hip.so).
 *
 * The reference (stevenmiller888/mlx-audio) has no FFI: its hot path sits behind plain Python
 * callables that dispatch every op to the MLX runtime.  This header is the boundary a maintainer
 * would bind instead (ctypes stub in INTEGRATION.md).  Each entry point names the reference
 * interface it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; kk_last_error() gives the message.
 *     No C++ exception crosses this boundary.
 *   - all data pointers are DEVICE pointers (hipMalloc / torch.cuda tensors) unless the parameter is
 *     documented as host memory.  The caller owns every buffer; the library never frees or keeps one
 *     beyond the call, except the weights it copied in kk_load_tensor/kk_finalize.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*) and is asynchronous; no entry
 *     point synchronises the device except kk_finalize.
 *   - a kk_model is IMMUTABLE after kk_finalize and may be shared by any number of threads / streams (one copy of the weights).  Everything a
 *     forward mutates -- the cache of captured graphs (kk_set_graph_mode), the side stream + fork / join events of a forward, the debug hooks
 *     and switches, the profile brackets -- lives in a kk_context, made by kk_context_create: ONE CONTEXT PER STREAM / THREAD in flight, each with its
 *     own caller-owned workspace (bench.py --streams, TTSService(replicas=...) share one model).  A context is not thread safe; the model is.
 *   - tensors are "frames-major": [B][L][C] with C contiguous.
 */
#ifndef KOKORO_HIP_H
#define KOKORO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KK_ABI_VERSION 2 /* 2: forward / graph / debug / profile entry points take a kk_context: round 3 */
#define KK_ABI_MINOR 29  /* additions that leave every entry point of the major version as it was; 1: quantised CSM checkpoints (kk_csm_load_quantized ...);
                            2: the full CSM sampler and its device RNG (kk_csm_sampler, kk_csm_generate_frame_ex, kk_op_csm_sample_ex, kk_op_csm_uniforms);
                            3: continuous batching of CSM streams (kk_csm_admit, kk_csm_park_row, kk_csm_shift_caches, kk_csm_row_state, kk_csm_reset_caches_parked);
                            4: shared voice prefixes of CSM streams (kk_csm_prefix_*, kk_csm_admit_prefixed);
                            5: row-mode streaming Mimi decode (kk_mimi_stream_create_rows, kk_mimi_stream_reset_row, kk_mimi_decode_step_rows,
                               kk_mimi_stream_row_frames, kk_mimi_stream_row_snapshot);
                            6: per-row sampler settings of a CSM batch (kk_csm_set_row_sampler, kk_csm_generate_frame_rows, kk_op_csm_sample_rows);
                            7: a prefix captured from a live cache row (kk_csm_prefix_capture);
                            8: a finished admission moved between two generators' cache rows (kk_csm_admit_transfer);
                            9: row-mode streaming Mimi ENCODE (kk_mimi_stream_create_rows_encoder, kk_mimi_encode_step_rows; kk_mimi_stream_reset_row,
                               kk_mimi_stream_row_frames, kk_mimi_stream_set_context and kk_mimi_stream_row_snapshot take either direction);
                            10: row-mode polyphase resampler (kk_resampler_create, kk_resampler_destroy, kk_resampler_set_row, kk_resampler_step,
                               kk_resampler_block_outputs, kk_op_resample);
                            11: PCM wire formats at the resampler's edges and on their own (KK_PCM_*, kk_resampler_set_row_fmt, kk_resampler_step_fmt,
                               kk_pcm_convert_rows, kk_op_pcm_convert);
                            12: row-mode voice-activity detector (kk_vad_create, kk_vad_destroy, kk_vad_set_row, kk_vad_step, kk_op_vad);
                            13: re-arming detector over a ring and row-table ring copies (kk_vad_ring_create, kk_vad_ring_destroy,
                               kk_vad_ring_set_row, kk_vad_ring_step, kk_ring_write_rows, kk_ring_read_rows);
                            14: Whisper's audio side (kk_op_log_mel, kk_op_attention_long, kk_whisper_create, kk_whisper_destroy, kk_whisper_load_tensor,
                               kk_whisper_finalize, kk_whisper_encode_workspace_bytes, kk_whisper_encode);
                            15: Whisper's text side (kk_op_whisper_attn_rows, kk_op_whisper_linear_rows, kk_op_whisper_embed, kk_op_whisper_pick,
                               kk_op_whisper_pick_reset, kk_whisper_text_*);
                            16: Whisper's token timestamps (kk_op_whisper_qk_rows, kk_op_whisper_align_matrix, kk_op_whisper_dtw with their
                               ..._workspace_bytes, kk_op_whisper_median_filter, kk_whisper_text_forward_qk, kk_whisper_text_qk_bytes);
                            17: the cache attention's block forms on caller-owned buffers (kk_op_attn_cache_block);
                            18: row mode of Whisper's text side (kk_whisper_text_rows_*, kk_whisper_rows_item, KK_WHISPER_MAX_ROWS);
                            19: the fused statistics' finalize / fold step on caller-owned buffers (kk_op_norm_finalize);
                            20: the Mimi codec's own kernels and its conv dispatch on caller-owned buffers (kk_op_mimi_conv, kk_op_mimi_rvq_sum,
                               kk_op_mimi_upsample, kk_op_mimi_rope, kk_op_mimi_conv_cout1, kk_op_mimi_edge_pad, kk_op_mimi_rvq_argmin,
                               kk_op_mimi_carry);
                            21: Whisper sampling: the sampled pick and window groups on one cross K/V slice (kk_op_whisper_pick_sampled,
                               kk_whisper_text_state_bytes_groups, kk_whisper_text_set_audio_groups,
                               kk_whisper_text_sample_setup, KK_WHISPER_MAX_GROUP);
                            22: the epilogue class of the fused conv kernels as a test switch and query (kk_debug_set_op_variant 41 / 51,
                               kk_debug_last_conv_epi, kk_debug_set_op_accumulate);
                            23: Whisper beam search on the device (kk_op_whisper_beam_topk, kk_op_whisper_beam_select, kk_op_whisper_beam_reset,
                               kk_op_whisper_attn_rows_owned, kk_whisper_beam_bufs, kk_whisper_text_beam_state_bytes, kk_whisper_text_beam_setup,
                               kk_whisper_text_beam_not_complete, kk_whisper_text_beam_read);
                            24: quantised Whisper checkpoints, decoder matrices packed in device memory (kk_whisper_text_load_quantized,
                               kk_whisper_text_weight_info, kk_whisper_text_weight_fallback, kk_op_whisper_linear_rows_q, kk_op_whisper_embed_q);
                            25: Whisper long-form transcription: a sampled pick per row of row mode and windows cut out of whole-file spectrograms
                               (kk_whisper_text_rows_set_draw, kk_op_mel_windows);
                            26: groups of row mode: beam search and best_of in the running batch (kk_whisper_text_rows_groups_state_bytes,
                               kk_whisper_text_rows_groups_bind, kk_whisper_text_rows_admit_group, kk_whisper_text_rows_group_read,
                               kk_whisper_text_rows_group_release, kk_whisper_text_rows_group_offers, KK_WHISPER_GROUP_PLAIN / _BEAM);
                            27: a listener's utterance becomes a Whisper window: spans of sample buffers, resampled and log-mel'ed in one launch pair
                               (kk_op_log_mel_spans);
                            28: the SNAC codec and its kernels on their own (kk_snac_*, kk_op_snac_dw_conv, kk_op_snac_residual_unit,
                               kk_op_snac_from_codes, kk_op_snac_vq_search, kk_op_snac_conv_cout1);
                            29: the Kokoro forward's glue kernels, the Albert embedding and the ragged source / STFT on caller-owned buffers
                               (kk_op_kokoro_style_fc, kk_op_kokoro_fill_style, kk_op_kokoro_embedding, kk_op_kokoro_duration, kk_op_kokoro_alignment,
                               kk_op_kokoro_gather_rows, kk_op_kokoro_copy_slice, kk_op_kokoro_lens, kk_op_kokoro_convert, kk_op_albert_embed,
                               kk_op_source_stft_ragged) */

enum { KK_DTYPE_F32 = 0, KK_DTYPE_BF16 = 1, KK_DTYPE_I32 = 2, KK_DTYPE_F16 = 3 };
enum { KK_NOISE_ZERO = 0, KK_NOISE_INJECTED = 1, KK_NOISE_PHILOX = 2 };

typedef struct kk_model kk_model;
typedef struct kk_context kk_context;

/* Hyper-parameters: mlx_audio/tts/models/kokoro/kokoro.py:47-63 (ModelConfig), values pinned by
 * mlx_audio/tts/tests/test_models.py:92-122; Albert defaults mlx_audio/tts/models/kokoro/modules.py:418-435. */
typedef struct kk_config {
  int32_t n_token, hidden_dim, style_dim, n_layer, max_dur, text_encoder_kernel_size;
  int32_t plbert_hidden, plbert_heads, plbert_intermediate, plbert_max_pos, plbert_layers, plbert_embedding;
  int32_t decoder_hidden;             /* 1024, hard-coded at istftnet.py:917-932 */
  int32_t upsample_initial_channel;
  int32_t n_upsamples;                /* 2 */
  int32_t upsample_rates[4];          /* 10, 6 */
  int32_t upsample_kernel_sizes[4];   /* 20, 12 */
  int32_t n_resblock_kernels;         /* 3 */
  int32_t resblock_kernel_sizes[4];   /* 3, 7, 11 */
  int32_t resblock_dilations[4][3];   /* {1,3,5} x3 */
  int32_t gen_istft_n_fft, gen_istft_hop_size; /* 20, 5 */
  int32_t compute_dtype;              /* KK_DTYPE_F32 (exact path) or KK_DTYPE_BF16 (MFMA path) */
} kk_config;

/* Model(config)  --  kokoro.py:83-113 */
int kk_create(const kk_config* cfg, kk_model** out);
void kk_destroy(kk_model* m);

/* model.load_weights(...) after Model.sanitize  --  mlx_audio/tts/utils.py:217-262, kokoro.py:172-252,
 * istftnet.py:965-979.  `name` is the MLX-side parameter name; `data` is HOST memory in `dtype`
 * (F32 / BF16 / F16).  Conv weights may arrive in either layout ([O,K,I] MLX or [O,I,K] PyTorch): the
 * library decides by the expected shape, not by the reference's check_array_shape heuristic
 * (mlx_audio/tts/models/base.py:21-34).  PyTorch-side LSTM / gamma / beta names are accepted too. */
int kk_load_tensor(kk_model* m, const char* name, int dtype, const int64_t* shape, int ndim, const void* host_data);

/* Folds weight_norm once (istftnet.py:53-93,130: g*v/(||v||+1e-7), recomputed per call in the
 * reference), packs every matrix for the kernels and uploads.  Fails if a parameter is missing.
 * Synchronises `stream`. */
int kk_finalize(kk_model* m, void* stream);

/* Bytes of scratch kk_forward* needs for a batch of B utterances of at most Tmax tokens (BOS/EOS
 * included) and Fmax frames (Fmax = 0: text stage only). */
size_t kk_workspace_bytes(const kk_model* m, int B, int Tmax, int Fmax);

/* The per-stream run state of a finalized model (the reference's Model is one object because its forward is single threaded:
 * kokoro.py:83-113 holds module state such as `_pipelines`, istftnet.py:526 caches the STFT).  Any number of contexts may share one model;
 * use one per stream / thread in flight.  kk_context_workspace_bytes is kk_workspace_bytes under THIS context's debug switches (some of them
 * materialise extra intermediates).  Destroy every context before kk_destroy(model). */
int kk_context_create(kk_model* m, kk_context** out);
void kk_context_destroy(kk_context* cx);
kk_model* kk_context_model(kk_context* cx);
size_t kk_context_workspace_bytes(const kk_context* cx, int B, int Tmax, int Fmax);

/* Text stage of Model.__call__  --  kokoro.py:135-150 and :159-161:
 *   Albert -> bert_encoder -> DurationEncoder -> duration LSTM/proj -> pred_dur ; TextEncoder.
 * ids      [B][Tmax] int32, zero padded, row b = [0, ids..., 0] (kokoro.py:135)
 * lens     [B] int32, tokens per utterance including the two zeros
 * ref_s    [B][256] float32 style rows (pipeline.py:236; [:128] decoder, [128:] prosody, kokoro.py:145,165)
 * speed    [B] float32
 * pred_dur_out [B][Tmax] int32  = clip(round(sum(sigmoid(.))/speed), 1) (kokoro.py:149-150), 0 past lens[b]
 * The stage's results stay in `workspace` for kk_forward_audio. */
int kk_forward_text(kk_context* cx, void* stream, int B, int Tmax, const int32_t* ids, const int32_t* lens, const float* ref_s,
                    const float* speed, void* workspace, size_t workspace_bytes, int32_t* pred_dur_out);

/* Audio stage of Model.__call__  --  kokoro.py:151-165: alignment, F0Ntrain, Decoder, Generator, iSTFT.
 * dur       [B][Tmax] int32 durations to realise (pred_dur_out, or forced ones)
 * Fmax      frame capacity per utterance; frames past it are dropped (nframes_out reports min(sum, Fmax))
 * noise_mode / sine_noise / seed : the reference draws N(0,1) at istftnet.py:620; KK_NOISE_INJECTED reads
 *           sine_noise [B][600*Fmax][9] float32, KK_NOISE_PHILOX generates it on the fly from `seed`.
 * wav_out   [B][600*Fmax] float32 (zeros past 600*nframes)   -- Output.audio, kokoro.py:165-170
 * nframes_out [B] int32 */
int kk_forward_audio(kk_context* cx, void* stream, int B, int Tmax, const int32_t* lens, const float* ref_s, const int32_t* dur, int Fmax,
                     int noise_mode, const float* sine_noise, uint64_t seed, void* workspace, size_t workspace_bytes, float* wav_out,
                     int32_t* nframes_out);

/* Model.__call__ in one call (kokoro.py:120-170) without the reference's mid-forward host sync
 * (kokoro.py:151-153): durations are `forced_dur` if non-null, else the predicted ones, realised on
 * device and truncated at Fmax frames. */
int kk_forward(kk_context* cx, void* stream, int B, int Tmax, const int32_t* ids, const int32_t* lens, const float* ref_s, const float* speed,
               const int32_t* forced_dur, int Fmax, int noise_mode, const float* sine_noise, uint64_t seed, void* workspace,
               size_t workspace_bytes, float* wav_out, int32_t* pred_dur_out, int32_t* nframes_out);

/* Graph replay of kk_forward (off by default).  With it on, the SECOND call with an identical argument tuple (every pointer,
 * B, Tmax, Fmax, noise_mode; the seed may differ) is captured into a hipGraph on `stream` and that call and all later ones
 * are ONE hipGraphLaunch instead of ~450 kernel launches; results are bit-identical to the eager call.  Calls with debug
 * overrides or an open profile run eagerly.  The reference has no counterpart (MLX builds its own lazy graph per call,
 * kokoro.py:120-170 is re-traced every time). */
int kk_set_graph_mode(kk_context* cx, int on);

/* load_model's quantization branch  --  mlx_audio/tts/utils.py:241-260 (nn.quantize with the class predicate of :349-369; BASELINE
 * config 5).  Call between kk_create and kk_finalize when config["quantization"] is present; the weights handed to kk_load_tensor are
 * the DEQUANTISED ones (scale * q + bias per group, mlx-audio_amd/quant.py).  With compute_dtype bf16 the quantised Linear set with
 * eligible shapes (inputs % 64 == 0, outputs % 64 == 0: Albert's embedding map / QKV / dense / ffn / ffn_output and bert_encoder,
 * 99.9 % of the quantised FLOPs) is re-quantised to OCP e4m3 with one power-of-two (E8M0) scale per `group_size` inputs and runs on
 * the block-scaled fp8 matrix instruction; activations are quantised per (row, 32 inputs) on the fly.  The remaining members of the
 * set (style `fc` layers, duration_proj, embeddings: M = batch rows or table lookups) use the dequantised weights in fp32.
 * bits must be 8.  kk_quantized_layers reports how many of the 6 linears got an fp8 pack (after kk_finalize). */
int kk_set_quantization(kk_model* m, int group_size, int bits);
int kk_quantized_layers(const kk_model* m);

const char* kk_last_error(void);
int kk_abi_version(void);
int kk_abi_minor(void);

/* ---- single-kernel entry points (used by the parity tests; same kernels kk_forward launches) ---- */

/* mx.conv1d / mx.conv_transpose1d / nn.Linear  --  istftnet.py:137-157.  w_packed [K][Cin][ldw] fp32 (device). */
int kk_op_conv1d(void* stream, int B, const void* x, int ldx, int Lin_rows, const int32_t* lin, const float* w_packed, int ldw,
                 const float* bias, int Cin, int Cout, int Kw, int transposed, int stride, int pad, int dil, int in_shift, float in_slope,
                 int act, float act_slope, const void* res, int ldr, float scale, int accumulate, void* out, int ldo, int Lout_rows,
                 const int32_t* lout, int in_dtype, int out_dtype);
/* the same ops on the bf16 MFMA kernel.  w_bf16 packed [Kw][CoutP][CinP] (CinP % 64 == 0, CoutP % 128 == 0, zero padded),
 * x bf16 with ldx >= CinP, out bf16 or fp32 (out_dtype), bias [CoutP]. */
int kk_op_conv1d_bf16(void* stream, int B, const void* x, int ldx, int Lin_rows, const int32_t* lin, const void* w_bf16, int CinP, int CoutP,
                      const float* bias, int Cout, int Kw, int transposed, int stride, int pad, int dil, int in_shift, float in_slope,
                      int act, float act_slope, const void* res, int ldr, float scale, int accumulate, void* out, int ldo, int Lout_rows,
                      const int32_t* lout, int out_dtype);
/* the fused resblock form of the bf16 path: y = act(x * nrm_a[b][c] + nrm_b[b][c]) applied while the input is staged
 * (AdaIN1d + Snake / LeakyReLU, istftnet.py:333-337,382) and per-tile column sums / sums of squares of the stored output
 * (stat_part [B][ntiles][2][Cout], the next InstanceNorm's statistics, istftnet.py:229-230) */
int kk_op_conv1d_bf16_fused(void* stream, int B, const void* x, int ldx, int L_rows, const int32_t* len, const void* w_bf16, int CinP,
                            int CoutP, const float* bias, int Cin, int Cout, int Kw, int pad, int dil, const float* nrm_a,
                            const float* nrm_b, int nrm_stride, int nrm_act, float nrm_slope, const float* nrm_alpha, const void* res,
                            int ldr, float scale, void* out, int ldo, float* stat_part, int* stat_ntiles_out);
/* InstanceNorm statistics + AdaIN1d + activation (+ pool)  --  istftnet.py:216-268,327-338,382,874-882
 * `scratch` (at least nchunk * B * 2 * C + 2 * B * C floats, nchunk = ceil(L_rows / 512)) holds on return:
 *   the partial sums  [B][nchunk][2][C]   (sum and sum of squares of x - x[b][0][c] over each 512-row chunk),
 *   then mean [B][C]  at offset B * nchunk * 2 * C,
 *   then rstd [B][C]  = 1 / sqrt(var + 1e-5), ddof 0; both 0 for an item of length 0. */
int kk_op_adain(void* stream, int B, const void* x, int ldx, int L_rows, const int32_t* len, int C, const float* gamma_beta, int gbs,
                int act, float slope, const float* alpha, int pool, const float* pool_w, const float* pool_b, void* out, int ldo, int Cpad,
                int Lout_rows, float* scratch, size_t scratch_floats, int dtype, int fast);
/* The tail of the fused statistics on caller-owned buffers: the step from the per-tile column sums that kk_op_conv1d_bf16_fused writes to the
 * next AdaIN's parameters (istftnet.py:229-230,333-337).  Two forms:
 *   finalize (partial != NULL): partial [B][ntiles][2][C] holds UN-shifted sums and sums of squares per tile; all ntiles tiles are summed in double,
 *     mean = S / n, var = max(SS / n - mean^2, 0), rstd = 1 / sqrt(var + 1e-5) with n = len[b] (L_rows for every item when len == NULL); an item
 *     of length 0 gets mean = rstd = 0.  mean / rstd [B][C] are written where given.  With add_row_bf16 (bf16, item b at add_row_bf16 +
 *     b * add_row_bs elements) row 0 of each item and its square are first added to tile 0 of `partial` in place, the other tiles stay as they are.
 *   fold (partial == NULL): mean / rstd [B][C] are inputs.
 * With pa / pb (both, and gamma_beta [B][gbs], gamma = [c], beta = [C + c]): pa[b * pstride + c] = rstd * (1 + gamma), pb = beta - mean * pa for
 * c < C, exactly 0 for C <= c < Cp, untouched from Cp on.  Refused before any launch: B, C or (finalize form) ntiles <= 0, pa without pb or without
 * gamma_beta, Cp < C, pstride < Cp, the fold form without mean / rstd / pa or with add_row_bf16. */
int kk_op_norm_finalize(void* stream, int B, int C, const int32_t* len, int L_rows, float* partial, int ntiles, const void* add_row_bf16,
                        long long add_row_bs, const float* gamma_beta, int gbs, float* mean, float* rstd, float* pa, float* pb, int pstride,
                        int Cp);
/* nn.LayerNorm / AdaLayerNorm  --  modules.py:33,71-90 */
int kk_op_layernorm(void* stream, int B, const void* x, int ldx, const void* res, int ldr, int L_rows, const int32_t* len, int C,
                    const float* w, const float* b, const float* gamma_beta, int gbs, float eps, int act, float slope, void* out, int ldo,
                    int dtype);
/* LSTM recurrence  --  modules.py:152-239 */
int kk_op_lstm(void* stream, int B, const float* xproj, const float* whT, int H, int L_rows, const int32_t* len, void* out, int ldo,
               int dtype);
/* the same recurrence for H = 256 with Wh given as bf16 [2][4H][H] (row = gate row, i|f|g|o) and kept on chip */
/* The streaming matrix-core Linear of the text side (kk_linear_rows.hip; Albert / bert_encoder / map_in Linears, modules.py:414-512, while few rows are in
 * flight) on its own: out[b][t][:] = act(x[b][t][:K] W^T + bias) for t < len[b], zeros past it.  x / out bf16 at item pitches xbs / obs elements and row
 * pitches ldx / ldo; w_bf16 [N][K] row-major bf16; pack_scratch: ceil(N / 16) * 16 * K bf16 of device memory; act 0 none, 2 exact-erf GELU. */
int kk_op_linear_rows(void* stream, int B, const void* x_bf16, long long xbs, int ldx, int rows, const int32_t* len, const void* w_bf16, int N, int K,
                      const float* bias, int act, void* pack_scratch, void* out_bf16, long long obs, int ldo);
int kk_op_lstm_bf16(void* stream, int B, const float* xproj, const void* wh_bf16, int L_rows, const int32_t* len, void* out, int ldo,
                    int dtype);
/* AlbertSelfAttention core  --  modules.py:497-512 */
int kk_op_attention(void* stream, int B, const void* qkv, int ld, int T_rows, const int32_t* len, int heads, void* out, int ldo, int dtype);
/* SourceModuleHnNSF + MLXSTFT.transform  --  istftnet.py:606-680,463-495 */
int kk_op_source_stft(void* stream, int B, const float* f0, int L2_rows, const int32_t* len2, const float* lin_w9, float lin_b,
                      int noise_mode, const float* noise, uint64_t seed, float* phase_scratch, float* har_source, void* har, int ldhar,
                      int dtype);
/* The same two launches with ragged lengths (tests): len2 [B] valid F0 entries (<= L2_rows) and lenN [B] valid samples (<= 300 * L2_rows) are
 * DEVICE pointers, each nullable (NULL = all of them).  The forward passes lenN = 300 * len2; here it is free, so the STFT's reflect padding can meet
 * an edge at any sample.  phase_scratch fp32 [B][9][L2_rows], har_source fp32 [B][300 * L2_rows] (zero from 300 * len2 on), har [B][60 * L2_rows + 1]
 * [ldhar >= 22]: magnitude at 0..10, angle at 11..21, rows from lenN / 5 + 1 on (all rows when lenN is 0) zero.  A signal shorter than the padding
 * (0 < lenN < 11), which the reference refuses, is folded back into range as numpy's reflect mode does. */
int kk_op_source_stft_ragged(void* stream, int B, const float* f0, int L2_rows, const int32_t* len2, const int32_t* lenN, const float* lin_w9,
                             float lin_b, int noise_mode, const float* noise, uint64_t seed, float* phase_scratch, float* har_source, void* har,
                             int ldhar, int dtype);
/* The glue kernels of the Kokoro forward (csrc/kk_misc.hip) and the Albert embedding on caller-owned buffers (tests).  Every entry makes the call
 * kk_forward makes.  Tensors are [B][rows][ld] with item pitch rows * ld; `len` [B] is a DEVICE pointer to the valid rows per item, NULL = all rows;
 * dtype is KK_DTYPE_F32 or KK_DTYPE_BF16 and names the element type of the void* tensors.  Refused before any launch: a null tensor, B or a row /
 * channel count < 1, a pitch smaller than the channels it must hold.
 *   style_fc     out[b][o] = sum_j wT[j][o] ref_s[b][soff + j] + bias[o], j < 128, o < N; ref_s fp32 [B][256], wT fp32 [128][N], soff in [0, 128]
 *   fill_style   out[b][t][coff + j] = ref_s[b][soff + j] for t < len[b], else 0; j < S, soff + S <= 256; other columns untouched
 *   embedding    out[b][t][c] = table[ids[b][t]][c] for t < len[b], else 0; ids int32 [B][T_rows] (not read past len), table fp32 [*][C]
 *   duration     d = sum_{o < nout} sigmoid(x[b][t][:Cin] . W[:, o] + bias[o]) / speed[b]; dur_f = d (nullable), dur = max(1, rint(d)) with ties to
 *                even; both 0 for t >= len[b].  W fp32 [Cin][nout], speed fp32 [B], dur int32 [B][T_rows]
 *   alignment    frame_idx[b][f] = the token t whose frames [sum_{u < t} max(dur_u, 0), + max(dur_t, 0)) hold f, over t < lenT[b]; lenF[b] =
 *                min(sum, F_rows); frame_idx is 0 from lenF[b] on.  lenT is required (DEVICE, [B]); T_rows > 512 is refused
 *   gather_rows  out[b][f][coff + c] = in[b][frame_idx[b][f]][c] for f < lenF[b], else 0; c < C; in [B][T_rows][ldi]; lenF is required
 *   copy_slice   out[b][l][coff + c] = in[b][l][c] for l < len[b], else 0
 *   lens         lens_out [4][B] = 2 F, 2 F up0, 2 F up0 up1 + 1 (0 when F = 0), 2 F up0 up1 hop, F = lenF[b] (required)
 *   convert      dst[b][r][c] = (dst type) src[b][r][c]: fp32 -> fp32, fp32 -> bf16 (round to nearest even), bf16 -> fp32; bf16 -> bf16 is refused
 *   albert_embed out[b][t][:E] = LayerNorm_eps(word[ids[b][t]] + pos[t] + type[0 row]) * ln_w + ln_b (modules.py:451-465) for t < len[b], else 0;
 *                tables fp32 [*][E]; E > 512 is refused */
int kk_op_kokoro_style_fc(void* stream, int B, const float* ref_s, int soff, const float* wT, const float* bias, float* out, int N);
int kk_op_kokoro_fill_style(void* stream, int B, const float* ref_s, int soff, void* out, int ldo, int coff, int S, int L_rows, const int32_t* len,
                            int dtype);
int kk_op_kokoro_embedding(void* stream, int B, const int32_t* ids, const float* table, void* out, int ldo, int C, int T_rows, const int32_t* len,
                           int dtype);
int kk_op_kokoro_duration(void* stream, int B, const void* x, int ldx, const float* W, const float* bias, int Cin, int nout, const float* speed,
                          int32_t* dur, float* dur_f, int T_rows, const int32_t* len, int dtype);
int kk_op_kokoro_alignment(void* stream, int B, const int32_t* dur, int T_rows, const int32_t* lenT, int32_t* frame_idx, int32_t* lenF, int F_rows);
int kk_op_kokoro_gather_rows(void* stream, int B, const void* in, int ldi, int T_rows, const int32_t* frame_idx, int F_rows, const int32_t* lenF,
                             void* out, int ldo, int coff, int C, int dtype);
int kk_op_kokoro_copy_slice(void* stream, int B, const void* in, int ldi, void* out, int ldo, int coff, int C, int L_rows, const int32_t* len,
                            int dtype);
int kk_op_kokoro_lens(void* stream, int B, const int32_t* lenF, int32_t* lens_out, int up0, int up1, int hop);
int kk_op_kokoro_convert(void* stream, int B, const void* src, int src_dtype, int lds, void* dst, int dst_dtype, int ldd, int C, int rows);
int kk_op_albert_embed(void* stream, int B, const int32_t* ids, const float* word, const float* pos, const float* type, const float* ln_w,
                       const float* ln_b, float eps, void* out, int ldo, int E, int T_rows, const int32_t* len, int dtype);
/* exp/sin + MLXSTFT.inverse + istft  --  istftnet.py:804-806,497-523; mlx_audio/utils.py:104-158 */
int kk_op_istft_head(void* stream, int B, const void* x, int ldx, int Tf_rows, const int32_t* len_frames, float* wav, int dtype, int fast);
/* The fused vocoder head of the bf16 mode: LeakyReLU(in_slope) -> conv_post (128 -> 22 channels, k = 7, pad 3) -> exp / sin -> inverse STFT ->
 * overlap-add, one kernel (istftnet.py:798-806,497-523; mlx_audio/utils.py:104-158).  x: bf16 [B][Tf_rows][ldx], 128 channels.
 * w_frag: conv_post in the kernel's fragment order, made by kk_op_pack_head_w from bf16 W[tap 7][cout 22][cin 128] (both DEVICE pointers,
 * w_frag holds 7 * 8 * 64 * 8 bf16).  cp_out (nullable): the conv_post tensor, bf16 [B][Tf_rows][cp_ld >= 22]. */
int kk_op_pack_head_w(void* stream, const void* w_bf16, void* w_frag);
int kk_op_conv_post_istft(void* stream, int B, const void* x, int ldx, int Tf_rows, const int32_t* len_frames, const void* w_frag,
                          const float* bias, float in_slope, float* wav, void* cp_out, int cp_ld);

/* MX-fp8 linear  --  the quantised nn.Linear of the reference's 8-bit checkpoints (mx.quantized_matmul, tts/utils.py:255-260).
 * kk_mxfp8_pack_weight (HOST to HOST): fp32 [N][K] -> e4m3 fragments + E8M0 scale bytes in MFMA fragment order, buffer sizes from
 * kk_mxfp8_bytes(N, K, ..).  kk_op_linear_mxfp8: x bf16 [M][ldx] (M = items * rows_per_item; len[item] valid rows, NULL = all) is
 * quantised into the caller's aq / as scratch (sizes kk_mxfp8_bytes(M, K, ..)), then out[m][n] = act(sum_k x[m][k] w[n][k] + bias[n])
 * in bf16, zero for rows past len.  act: 0 none, 2 exact GELU. */
int kk_mxfp8_bytes(int rows, int K, size_t* q_bytes, size_t* s_bytes);
int kk_mxfp8_pack_weight(const float* w_host, int N, int K, int group, uint8_t* q_host, uint8_t* s_host);
int kk_op_linear_mxfp8(void* stream, const void* x_bf16, int ldx, int M, int rows_per_item, const int32_t* len, int K, const void* wq,
                       const void* ws, int N, const float* bias, int act, void* aq, void* as, void* out_bf16, int ldo);

/* ---- debug hooks (tests only; not thread safe) ----
 * Named intermediates of the last kk_forward*: "bert_dur" "d" "t_en" "en" "asr" "F0_pred" "N_pred" "dec_out"
 * "har_source" "har" "gen_pre_res0" "gen_stage0" "gen_pre_res1" "gen_stage1" "conv_post".
 * Data format: dense float32 [B][rows][C] on the device. */
int kk_debug_info(kk_context* cx, const char* name, int64_t* rows, int64_t* channels);
int kk_debug_fetch(kk_context* cx, void* stream, const char* name, float* dst);
int kk_debug_override(kk_context* cx, const char* name, const float* src); /* src must stay valid until kk_debug_clear */
void kk_debug_clear(kk_context* cx);
/* variant 4 of the bf16 conv kernel reads its weights in MFMA fragment order: kk_op_pack_w_frag re-lays a [Kw][CoutP][CinP] bf16
 * pack out (device to device, same size); kk_debug_set_op_wfrag(wf) makes the kk_op_conv1d_bf16* calls that follow run variant 4
 * with that pack (NULL = back to the LDS-staged kernel).  The model packs both layouts in kk_finalize. */
int kk_op_pack_w_frag(void* stream, const void* w_bf16, void* w_frag, int Kw, int CoutP, int CinP);
void kk_debug_set_op_wfrag(const void* w_frag);
void kk_debug_set_op_accumulate(int on); /* kk_op_conv1d_bf16_fused with fragment-order weights adds its result to the output rows, as the last conv of a resblock adds to the mean over the three resblocks (0 = off, the default) */
int kk_debug_last_conv_epi(void); /* epilogue class of the latest variant-4 / 5 conv launch of this process: -1 = the generic instantiation (every choice a runtime branch), else the compiled-in mask 1 residual | 2 scale != 1 | 4 final LeakyReLU | 8 statistics | 16 read-and-add (variant 4) */
void kk_debug_set_op_variant(int v); /* 41 / 51: variant 4 / 5 with the generic epilogue instantiation also where a compiled-in class exists (the reference path of tests/test_gpu_conv_slim.py); 4 (default), 5 or 40: which fragment-order kernel those calls use (5 = wave-specialised persistent, kk_conv_mfma5.hip; 40 = variant 4 slab by slab also where its whole-K form (stride 1, 128 padded input channels) or its ring form (192 or more) applies -- the reference path of those forms' tests) */
void kk_debug_set_op_post_slope(float slope); /* LeakyReLU(slope) of the final stored value in the kk_op_conv1d_bf16* calls that follow (variants 4 / 5; 0 or 1 = none, the default) */
void kk_debug_force_generic(kk_context* cx, int flags); /* A/B tests in bf16 mode: bit0 no MFMA kernel, bit1 MFMA without norm fusion, bit2 LDS-staged MFMA kernel instead of variant 4, bit3 quantised model without the fp8 kernel, bit4 also materialise tensors fused kernels skip, bit5 stand-alone conv_post + iSTFT kernels, bit6 variant-5 (wave-specialised persistent) conv kernel wherever eligible, bit7 never (default: the layers with >= 9 taps), bit8 no side stream (the TextEncoder / harmonic-source branches of a forward on the caller's stream too), bit9 Linear layers never on the streaming kernel, bit10 always (default: by the rows in flight), bit11 conv variant 4 slab by slab also where its whole-K or ring form is routed (128 / 192 or more padded input channels; part of the graph-cache key like every bit) */

/* ---- per-kernel-class timing (bench.py): HIP events around every launch on the forward's stream ----
 * classes: 0 conv_generic 1 conv_mfma 2 instnorm_stats 3 adain_act 4 lstm 5 istft_head 6 layernorm 7 attention
 *          8 source 9 stft 10 linear_mxfp8.  kk_profile_end returns summed milliseconds, algorithmic flops / bytes and launch counts. */
int kk_profile_begin(kk_context* cx, int max_launches);
int kk_profile_end(kk_context* cx, int ncls, double* ms, double* flops, double* bytes, int64_t* count);

/* =====================================================================================================================
 * Mimi codec, decode path (CSM row C4): Mimi.decode, mlx_audio/codec/models/mimi/mimi.py:147-154.
 * Same conventions as above: device pointers, caller-owned buffers, work enqueued on `stream`, 0 = OK.
 * ===================================================================================================================== */
typedef struct kk_mimi kk_mimi;

/* mimi_202407 (mimi.py:41-101): dim 512, nq 32, bins 2048, qdim 256, 8 heads, 8 layers, ff 2048, nfilters 64,
 * ratios {8,6,5,4}, ksize 7, residual_ksize 3, last_ksize 3, upsample_stride 2, compress 2, rope_base 10000 */
typedef struct kk_mimi_config {
  int32_t dim, nq, bins, qdim, num_heads, num_layers, dim_feedforward, nfilters;
  int32_t n_ratios, ratios[8];
  int32_t ksize, residual_ksize, last_ksize, upsample_stride, compress;
  float rope_base;
  int32_t compute_dtype; /* KK_F32: parity path (generic fp32 kernels); KK_BF16: bf16 activations, variant-4 MFMA convolutions */
} kk_mimi_config;

int kk_mimi_create(const kk_mimi_config* cfg, kk_mimi** out);
void kk_mimi_destroy(kk_mimi* m);
/* parameters by their MLX-side names (after Mimi.load_pytorch_weights' remap, mimi.py:184-249), host fp32, MLX layouts:
 * conv / conv-transpose weights [O][K][I], code books as embedding_sum [bins][qdim] + cluster_usage [bins] */
int kk_mimi_load_tensor(kk_mimi* m, const char* name, const int64_t* shape, int ndim, const float* data);
int kk_mimi_finalize(kk_mimi* m, void* stream); /* code books divided by max(usage, 1e-5) (quantization.py:25-28), LayerScale folded, upload */
int64_t kk_mimi_samples_per_frame(const kk_mimi* m); /* 1920 for mimi_202407 */
size_t kk_mimi_workspace_bytes(kk_mimi* m, int B, int Nf);
/* codes [B][nq][Nf] int32 (device) -> pcm [B][samples_per_frame * Nf] float32 (device).  Like the reference's non-streaming
 * decode the transformer attends over the WHOLE sequence (no mask reaches the attention call, transformer.py:171). */
int kk_mimi_decode(kk_mimi* m, void* stream, int B, int Nf, const int32_t* codes, void* workspace, size_t workspace_bytes, float* pcm_out);
/* Mimi.encode (mimi.py:138-145): pcm [B][N] float32 -> codes [B][nq][kk_mimi_encode_frames(N)] int32.  Needs the
 * encoder.*, encoder_transformer.*, downsample.*, quantizer.*.input_proj parameters; always runs on the fp32 kernels (the
 * code-book search is an argmin). */
int kk_mimi_encode_frames(const kk_mimi* m, int N); /* ceil chain over the ratios and the resampler: 120000 -> 63 */
size_t kk_mimi_encode_workspace_bytes(kk_mimi* m, int B, int N);
int kk_mimi_encode(kk_mimi* m, void* stream, int B, int N, const float* pcm, void* workspace, size_t workspace_bytes, int32_t* codes_out);
/* Streaming: Mimi.decode_step / Mimi.encode_step / MimiStreamingDecoder (mimi.py:156-168,264-306; conv.py:265-351; seanet.py:219-223,277-283).
 * A stream owns the state the reference's streaming modules own, in device memory: per causal convolution the last k - stride input rows
 * (StreamableConv1d._prev_xs), per transposed convolution (k = 2 stride) the previous input row -- one row that determines the stride rows
 * of partial sums StreamableConvTranspose1d._prev_ys keeps --, the resampler's previous frame, and the KV caches of the transformer (last
 * 250 cached positions + the step's own, no mask: transformer.py:79-104).  Each step runs every layer over the rows of `chunk_frames` code
 * frames only.  decode: codes [B][nq][chunk] int32 -> pcm [B][chunk * samples_per_frame]; encode: the reverse.  fp32 kernels; B is fixed
 * between resets; at most max_frames frames per reset; a stream is created for one direction. */
typedef struct kk_mimi_stream kk_mimi_stream;
int kk_mimi_stream_create(kk_mimi* m, int max_batch, int max_frames, kk_mimi_stream** out); /* decode, one frame per step */
int kk_mimi_stream_create_chunked(kk_mimi* m, int encoder, int max_batch, int max_frames, int chunk_frames, kk_mimi_stream** out);
void kk_mimi_stream_destroy(kk_mimi_stream* s);
int kk_mimi_stream_reset(kk_mimi_stream* s); /* MimiStreamingDecoder.reset / Mimi.reset_state (mimi.py:131-137) */
int kk_mimi_stream_frames(const kk_mimi_stream* s);
int kk_mimi_stream_chunk_frames(const kk_mimi_stream* s);
/* the reference's step functions accept any number of frames per call and continue the state (mimi.py:156-168): frames per step of the
   following calls, 1 .. the chunk_frames the stream was created with */
int kk_mimi_stream_set_chunk(kk_mimi_stream* s, int chunk_frames);
int kk_mimi_stream_max_chunk_frames(const kk_mimi_stream* s);
int kk_mimi_stream_set_context(kk_mimi_stream* s, int context); /* TransformerConfig.context, default 250 (mimi.py:55-77); fresh / reset stream only */
size_t kk_mimi_stream_workspace_bytes(kk_mimi_stream* s, int B);
int kk_mimi_decode_step(kk_mimi_stream* s, void* stream, int B, const int32_t* codes, void* workspace, size_t workspace_bytes, float* pcm_out);
int kk_mimi_encode_step(kk_mimi_stream* s, void* stream, int B, const float* pcm, void* workspace, size_t workspace_bytes, int32_t* codes_out); /* Mimi.encode_step (mimi.py:156-161) */
/* Row mode (ABI minor 5): a decode stream whose rows each have their own position and lifetime, for a codec that follows a continuously
 * batched generator.  Positions live on the device (one int per row); a host mirror of the per-row frame counts carries every bound check,
 * so a refusal happens before any launch.  kk_mimi_decode_step_rows takes F <= max_chunk frames for ALL max_batch rows
 * (codes [max_batch][nq][F] on the device, active [max_batch] on the HOST); rows with active[b] == 0 ride along: their carried state, their
 * K / V below their position and their position are bit-unchanged, their pcm is finite and meaningless, their code entries may hold anything.
 * An active row's pcm is, bit for bit, that of a batch-1 kk_mimi_decode_step stream fed the same codes in the same step sizes.
 * kk_mimi_stream_reset_row starts one row over (one launch in stream order, no other row touched).  kk_mimi_decode_step, kk_mimi_stream_reset
 * and the encoder are refused on such a stream; kk_mimi_stream_set_context needs every row fresh; workspace: kk_mimi_stream_workspace_bytes(s, max_batch).
 * kk_mimi_stream_row_snapshot (tests): the row's device position (transformer rows), carried rows and K / V below the position, to the host. */
int kk_mimi_stream_create_rows(kk_mimi* m, int max_batch, int max_frames, int max_chunk, kk_mimi_stream** out);
int kk_mimi_stream_reset_row(kk_mimi_stream* s, void* stream, int row);
int kk_mimi_stream_row_frames(const kk_mimi_stream* s, int row);
int kk_mimi_decode_step_rows(kk_mimi_stream* s, void* stream, int F, const int32_t* codes, const int32_t* active, void* workspace, size_t workspace_bytes, float* pcm_out);
int kk_mimi_stream_row_snapshot(kk_mimi_stream* s, void* stream, int row, int32_t* pos_out, float* dst, size_t dst_floats, size_t* floats_out);
/* Row mode of the ENCODER (ABI minor 9): the same stream object for Mimi.encode_step, for microphones that start and stop on their own.  The
 * checkpoint must hold encoder.* parameters.  kk_mimi_encode_step_rows takes F <= max_chunk frames of pcm for ALL max_batch rows
 * (pcm [max_batch][F * samples_per_frame] float32 on the device, active [max_batch] on the HOST) and writes codes [max_batch][nq][F].  An
 * active row's codes equal, as integers, those of a fresh batch-1 kk_mimi_encode_step stream fed the same pcm in the same step sizes, whatever
 * the other rows do.  The resampler's 'edge' left padding is per row: an active row at position 0 (new, or after kk_mimi_stream_reset_row) has
 * its carried rows filled from its own first new row; no other row is touched.  An inactive row's pcm may hold anything (NaN, inf): nothing of
 * it reaches another row or its own carried rows, K / V and position; its code entries are unspecified and written in range.  Every bound
 * (frames per row, F, workspace, direction) is checked on the host before any launch.  kk_mimi_decode_step_rows on an encoder stream,
 * kk_mimi_encode_step_rows on a decoder stream and kk_mimi_encode_step on a row-mode stream are refused.  kk_mimi_stream_row_snapshot holds the
 * K / V of the encoder's layers for such a stream. */
int kk_mimi_stream_create_rows_encoder(kk_mimi* m, int max_batch, int max_frames, int max_chunk, kk_mimi_stream** out);
int kk_mimi_encode_step_rows(kk_mimi_stream* s, void* stream, int F, const float* pcm, const int32_t* active, void* workspace, size_t workspace_bytes, int32_t* codes_out);
/* intermediates of the last decode / encode (tests): "quantized", "upsampled", "transformer", "layer0".."layer3" (decode), "seanet", "transformer", "downsampled" (encode); [B][rows][channels] fp32 */
int kk_mimi_debug_info(kk_mimi* m, const char* name, int64_t* rows, int64_t* channels);
int kk_mimi_debug_fetch(kk_mimi* m, void* stream, const char* name, float* dst);

/* ---- the codec's kernels on their own (ABI minor 20; single-kernel entry points as above: device pointers, caller-owned buffers, work enqueued
 * on `stream`, 0 = OK; every bad argument is refused on the host before any launch with a kk_last_error() text).  Tensors are frames-major
 * [B][rows][ld]; dtypes are KK_DTYPE_F32 / KK_DTYPE_BF16; pitches count elements.  These call the launch functions the codec calls. */
enum { KK_MIMI_CONV_GENERIC = 0, KK_MIMI_CONV_FEW_ROWS = 1, KK_MIMI_CONV_MFMA = 2 };           /* *path_out of kk_op_mimi_conv */
enum { KK_MIMI_COUT1_F32 = 0, KK_MIMI_COUT1_BF16 = 1, KK_MIMI_COUT1_BF16_STAGED = 2 };         /* *form_out of kk_op_mimi_conv_cout1 */
enum { KK_MIMI_CARRY_SHIFT = 0, KK_MIMI_CARRY_EDGE_FILL = 1, KK_MIMI_CARRY_EDGE_FILL_ROWS = 2, KK_MIMI_CARRY_SHIFT_ROWS = 3,
       KK_MIMI_CARRY_RESET_ROW = 4, KK_MIMI_CARRY_SET_ACTIVE = 5 };                             /* op of kk_op_mimi_carry */
/* The codec's conv / transposed conv / linear dispatch (every convolution and Linear of kk_mimi_decode / encode and their steps goes through
 * it) on the caller's tensors and weights; *path_out says which kernel it launched (-1 when refused):
 *   KK_MIMI_CONV_MFMA      the variant-4 matrix-core kernel: w_frag given, x and out bf16, ldx >= CinP, shape eligible (Cout % 8 == 0,
 *                          Cin, Cout >= 16, stride 1 unless transposed, halo within the kernel's);
 *   KK_MIMI_CONV_FEW_ROWS  the weight-streaming kernel of the streaming steps: fp32 in and out, pad 0, dil 1, Cout >= 32, ldx == Cin, and either
 *                          stride 1 with x_rows == out_rows + Kw - 1 and out_rows <= 128 (linear / causal conv over contiguous rows), or
 *                          transposed with Kw == 2 * stride, out_rows == x_rows * stride, 2 <= x_rows <= 129, no res, no accumulate (row 0 of x is
 *                          the carried previous input row: output rows [0, stride) are NOT written); in_act = ELU runs a pre-pass into elu_tmp,
 *                          which must hold B * x_rows * ldx floats: a smaller one is refused, and only when this kernel is the one taken (no
 *                          other path reads elu_tmp); without elu_tmp (NULL, elu_floats 0 -- they come together) such a call goes to the
 *                          generic kernel;
 *   KK_MIMI_CONV_GENERIC   everything else (kk_op_conv1d's kernel, here with in_act and stride > 1).
 * out[b][q] = act(bias + sum_k sum_c in_act(x[b][q * stride - pad + k * dil][c]) w[k][c][:]) (+ res[b][q]) (+ old out when accumulate);
 * transposed: out[b][p] sums w[k] x[b][(p + pad - k) / stride] over the k with an integral row; rows outside [0, x_rows) are zeros.
 * w_packed [Kw][Cin][ldw] fp32 (ldw % 4 == 0, >= Cout rounded up to 64; columns >= Cout are never used).  w_frag (optional): the bf16 pack
 * [Kw][CoutP][CinP] in fragment order (kk_op_pack_w_frag), CinP % 64 == 0, CoutP % 128 == 0; bias then has CoutP entries and must be given;
 * with w_frag, bf16 x / out / res need pitches that are multiples of 8 and 16-byte aligned pointers.  Channels [Cin, ldx) of x are never used.
 * x: item pitch xbs >= x_rows * ldx; out and res (res has out's dtype and row count) likewise.  in_act: 0 or 5 (ELU); act: 0 or 4 (tanh-GELU). */
int kk_op_mimi_conv(void* stream, int B, const void* x, long long xbs, int ldx, int x_rows, int x_dtype, const float* w_packed, int ldw,
                    const void* w_frag, int CinP, int CoutP, const float* bias, int Cin, int Cout, int Kw, int pad, int dil, int transposed,
                    int stride, int in_act, int act, const void* res, long long rbs, int ldr, int accumulate, void* out, long long obs, int ldo,
                    int out_rows, int out_dtype, float* elu_tmp, size_t elu_floats, int* path_out);
/* split-RVQ decode (quantization.py:97-101): codes [B][nq][Nf] int32 (clamped into [0, bins)), codebooks [nq][bins][qdim] fp32 ->
 * q_first [B][Nf][ld] = row of code book 0, q_rest = the sum of the rows of code books 1 .. nq-1 in ascending order in fp32 (zeros when nq == 1).
 * Columns [qdim, ld) are not written. */
int kk_op_mimi_rvq_sum(void* stream, int B, const int32_t* codes, const float* codebooks, int nq, int bins, int qdim, int Nf, int ld, void* q_first,
                       void* q_rest, int dtype);
/* depth-wise causal transposed conv, kernel 2 s, stride s (conv.py:82-95,379-401): x [B][Lin][ld] at item pitch xbs, w [2 s][C] fp32 ->
 * out [B][Lin * s][ld] dense; out[s t + j] = x[t] w[j] + x[t - 1] w[j + s] (the second term only for t > 0).  Columns [C, ld) are not written. */
int kk_op_mimi_upsample(void* stream, int B, const void* x, long long xbs, const float* w, int C, int ld, int Lin, int s, void* out, int dtype);
/* nn.RoPE(traditional) in place on the q and k thirds of qkv [B][T][ld] (ld >= 3 D): pairs (2 i, 2 i + 1) of every head of size hd rotated by
 * t * inv_freq[i], inv_freq [hd / 2] fp32.  The v third and columns >= 3 D are not touched. */
int kk_op_mimi_rope(void* stream, int B, int T, int D, int ld, int hd, const float* inv_freq, void* qkv, int dtype);
/* SEANet's last conv, Cout = 1 (seanet.py:258-268): out[b][t] = bias[0] + sum_k sum_c elu?(x[b][t - pad + k][c]) w_packed[(k Cin + c) ldw], rows
 * outside [0, L) are zeros; x [B][L][ld] dense, out [B][L] fp32.  Kw * Cin <= 8192.  *form_out: which of the three kernels ran
 * (KK_MIMI_COUT1_BF16_STAGED: bf16, Cin % 8 == 0, Cin <= 64, ld % 8 == 0, Kw <= 16; it rounds elu(x) to bf16 while staging). */
int kk_op_mimi_conv_cout1(void* stream, int B, const void* x, int dtype, int ld, int L, int Cin, int Kw, int pad, const float* w_packed, int ldw,
                          const float* bias, int elu, float* out, int* form_out);
/* mx.pad(mode="edge") of the resampler (conv.py:350-367): out [B][Lp][C] row p = x [B][L][C] row clamp(p - left, 0, L - 1); fp32, dense */
int kk_op_mimi_edge_pad(void* stream, int B, const float* x, int L, int C, int left, int Lp, float* out);
/* EuclideanCodebook.encode + the residual update (quantization.py:35-39,84-92): dots [B][T][bins], c2 [bins], codebook [bins][qdim] ->
 * codes[(b nq + cbi) T + t] = argmin_j (c2[j] - dots[j]) in fp32, the first index on ties, NaN distances skipped, bins - 1 when none is below
 * +inf; residual [B][T][qdim] -= codebook[code] in fp32.  No other entry of codes is written. */
int kk_op_mimi_rvq_argmin(void* stream, int B, const float* dots, const float* c2, const float* codebook, int bins, int qdim, int T, int nq, int cbi,
                          float* residual, int32_t* codes);
/* The streaming state's carry kernels.  A buffer i is bufs[i] (device) = [B items at pitch[i]][S[i] carried rows | new rows][C[i]] fp32; bufs, S, n,
 * C, pitch are HOST arrays of nbuf entries (nbuf == 1 except for the two table ops).  B is the number of items / rows.  Arguments an op does not
 * name are ignored by it.  Every op but SET_ACTIVE needs nbuf >= 1 and, per buffer, a non-null pointer, S, n, C >= 1 and
 * pitch >= (S + n) * C -- for the two table ops n counts rows per code frame, F >= 1 is required and the check is pitch >= (S + n * F) * C.
 * (S == 0 is refused: the codec never launches a carry for a buffer without carried rows.)
 *   SHIFT            (bufs, S, n, C, pitch; nbuf == 1)  rows [n, n + S) -> [0, S) of every item (they overlap when n < S); refused when
 *                    S * C > 8192 or when pitch is not a multiple of C
 *   EDGE_FILL        (bufs, S, n, C, pitch; nbuf == 1)  rows [0, S) = row S of every item
 *   EDGE_FILL_ROWS   (the same + active, pos: device int32 [B], both required)  the fill for the items with active[b] != 0 and pos[b] == 0 only
 *   SHIFT_ROWS       (bufs, S, n, C, pitch of nbuf >= 1 buffers, table_dev, active, pos, F, pos_step)  every buffer of the table, items with
 *                    active[b] != 0 only: rows [F n, F n + S) -> [0, S), then pos[b] += pos_step ONCE per item; inactive items and their pos
 *                    are not touched; refused when a buffer has S * C > 8192
 *   RESET_ROW        (the same table arguments, F as for SHIFT_ROWS, row in [0, B))  rows [0, S) of item `row` in every buffer = 0, pos[row] = 0
 *   SET_ACTIVE       (active, mask; no buffer)  active[b] = bit b of mask, b < B <= 64
 * The table ops need table_dev (nbuf * 32 bytes, device), active and pos; they upload the table to table_dev after synchronising `stream`. */
int kk_op_mimi_carry(void* stream, int op, int B, int nbuf, float* const* bufs, const int* S, const int* n, const int* C, const long long* pitch,
                     void* table_dev, int32_t* active, int32_t* pos, int F, int pos_step, int row, unsigned long long mask);

/* =====================================================================================================================
 * SNAC codec (ABI minor 28): mlx_audio/codec/models/snac/{snac,layers,vq}.py, the tokeniser / vocoder of the reference's Llama
 * TTS family.  Same conventions: device pointers, caller-owned buffers, work enqueued on `stream`, 0 = OK.  The reference's port is
 * restated as written: transposed convs without output padding (an odd stride s turns L rows into L s - 1), NoiseBlock noise of shape
 * [B][1][C] (one normal per item and channel), a no-op residual crop, snake(x) = x + sin^2(alpha x) / (alpha + 1e-9).
 * ===================================================================================================================== */
typedef struct kk_snac kk_snac;

/* SNAC.__init__ (snac.py:16-65).  snac_24khz: encoder_dim 48, encoder_rates {2,4,8,8}, latent_dim 768, decoder_dim 1024, decoder_rates
 * {8,8,4,2}, codebook_size 4096, codebook_dim 8, vq_strides {4,2,1}, noise 1, depthwise 1, attn_window_size 0 (None).
 * A non-zero attn_window_size (LocalMHA) and depthwise 0 are refused by kk_snac_create. */
typedef struct kk_snac_config {
  int32_t sampling_rate, encoder_dim, n_encoder_rates, encoder_rates[8], latent_dim, decoder_dim, n_decoder_rates, decoder_rates[8];
  int32_t attn_window_size, codebook_size, codebook_dim, n_vq, vq_strides[8], noise, depthwise;
  int32_t compute_dtype; /* of DECODE: KK_DTYPE_F32 (parity path) or KK_DTYPE_BF16 (bf16 activations, matrix-core dense convs); encode is always fp32 */
} kk_snac_config;

int kk_snac_create(const kk_snac_config* cfg, kk_snac** out);
void kk_snac_destroy(kk_snac* m);
/* parameters by the reference's names and layouts, host fp32: WNConv1d weight_g [O][1][1] / weight_v [O][K][I / groups] / bias [O],
 * WNConvTranspose1d weight_g [I][1][1] / weight_v [I][K][O], Snake alpha [1][C][1], codebook.weight [bins][dim] */
int kk_snac_load_tensor(kk_snac* m, const char* name, const int64_t* shape, int ndim, const float* data);
/* folds weight norm (g v / |v| over the axes except 0, float64), L2-normalises the code books for the search, makes the from_codes tables
 * out_proj(codebook) [bins][latent_dim] and the summed out_proj biases, packs and uploads.  Fails with the name of a missing parameter. */
int kk_snac_finalize(kk_snac* m, void* stream);
int64_t kk_snac_hop_length(const kk_snac* m);          /* prod(encoder_rates): 512 for snac_24khz */
int64_t kk_snac_decode_samples(const kk_snac* m, int T); /* samples per item of a decode of T latent frames (the chain of transposed-conv lengths) */
size_t kk_snac_decode_workspace_bytes(kk_snac* m, int B, int T);
/* SNAC.decode (snac.py:101-104).  codes: HOST array of n_vq device pointers, codes[i] int32 [B][T / vq_strides[i]] (clamped into range); T must be a
 * multiple of every stride.  noise: HOST array of one device pointer per decoder block, noise[l] fp32 [B][C_l] with C_l = decoder_dim >> (l + 1);
 * required when the model has NoiseBlocks, ignored otherwise.  pcm_out fp32 [B][kk_snac_decode_samples].  An item's samples do not depend on B
 * or on its place in the batch. */
int kk_snac_decode(kk_snac* m, void* stream, int B, int T, const int32_t* const* codes, const float* const* noise, void* workspace,
                   size_t workspace_bytes, float* pcm_out);
/* SNAC.encode (snac.py:95-99) after preprocess: pcm fp32 [B][N] -> codes_out (HOST array of n_vq device pointers) int32 [B][T / vq_strides[i]],
 * T = kk_snac_encode_frames.  Always fp32.  N must give a T that is a multiple of every stride (the caller pads as SNAC.preprocess does). */
int kk_snac_encode_frames(const kk_snac* m, int N);
size_t kk_snac_encode_workspace_bytes(kk_snac* m, int B, int N);
int kk_snac_encode(kk_snac* m, void* stream, int B, int N, const float* pcm, void* workspace, size_t workspace_bytes, int32_t* const* codes_out);
/* intermediates of the last decode / encode (tests), [B][rows][channels] fp32: "z_q", "block0" .. (decode); "encoder", "residual0" .. (the
 * residual after quantiser i) (encode) */
int kk_snac_debug_info(kk_snac* m, const char* name, int64_t* rows, int64_t* channels);
int kk_snac_debug_fetch(kk_snac* m, void* stream, const char* name, float* dst);

/* ---- the codec's kernels on their own (single-kernel entry points as above; these call the launch functions the codec calls).  Tensors are
 * frames-major [B][rows][ld]; dtypes are KK_DTYPE_F32 / KK_DTYPE_BF16 with fp32 arithmetic; pitches count elements. */
enum { KK_SNAC_UNIT_GENERIC = 0, KK_SNAC_UNIT_MFMA = 1 }; /* *path_out of kk_op_snac_residual_unit: the kernel of its 1x1 conv */
/* depth-wise dilated conv, 7 taps, pad 3 dil, 1 <= dil <= 9, a Snake on either side when its alpha [C] is given:
 * out[t][c] = snake_out?(sum_k w[c][k] snake_in?(x[t - 3 dil + k dil][c]) + bias[c]); rows outside [0, L) are zeros and are never read.
 * w [C][7], bias [C] fp32.  Columns [C, ldo) of out are not written. */
int kk_op_snac_dw_conv(void* stream, int B, const void* x, long long xbs, int ldx, int dtype, int L, int C, int dil, const float* w, const float* bias,
                       const float* alpha_in, const float* alpha_out, void* out, long long obs, int ldo);
/* ResidualUnit (layers.py:208-231): out = x + W snake(dw7(snake(x))) + b on dense items x [B][L][ldx], out [B][L][ldo]; tmp [B][L][ldx] holds the
 * depth-wise result between the two launches.  pw_packed [1][C][ldw] fp32; pw_frag (optional): the bf16 fragment pack [1][CoutP][CinP]
 * (kk_op_pack_w_frag), used for bf16 tensors with an eligible shape (C % 8 == 0, C >= 16), pw_bias then has CoutP entries. */
int kk_op_snac_residual_unit(void* stream, int B, const void* x, int ldx, int dtype, int L, int C, int dil, const float* dw_w, const float* dw_b,
                             const float* alpha1, const float* alpha2, const float* pw_packed, int ldw, const void* pw_frag, int CinP, int CoutP,
                             const float* pw_bias, void* tmp, void* out, int ldo, int* path_out);
/* from_codes (vq.py:109-129): out[b][t][c] = sum_i tables[i][codes[i][b][t / strides[i]]][c] + bias_sum[c], quantisers in ascending order in fp32,
 * codes clamped into [0, bins).  codes, strides, tables: HOST arrays of nq <= 8 entries (device pointers / ints); tables[i] fp32 [bins][D]. */
int kk_op_snac_from_codes(void* stream, int B, int T, int D, int nq, const int32_t* const* codes, const int32_t* strides, const float* const* tables,
                          int bins, const float* bias_sum, void* out, int ldo, int dtype);
/* decode_latents (vq.py:62-77) + the straight-through line: e = ze / max(|ze|, 1e-12), dist_j = |e|^2 - 2 e . codebook_n[j] + c2[j] in fp32,
 * codes[b][t] = the first index of the smallest distance, zq[b][t] = ze + (codebook[code] - ze).  ze [B][T][ldz], codebook / codebook_n
 * [bins][cd] (cd <= 64), c2 [bins], zq [B][T][ldq]; all fp32. */
int kk_op_snac_vq_search(void* stream, int B, int T, const float* ze, int ldz, int cd, const float* codebook, const float* codebook_n, const float* c2,
                         int bins, int32_t* codes, float* zq, int ldq);
/* the decoder's last conv, Cout = 1: out[b][t] = tanh?(sum_k sum_c snake?(x[b][t - pad + k][c]) w_packed[(k Cin + c) ldw] + bias[0]); rows outside
 * [0, L) are zeros; x [B][L][ld] dense, out [B][L] fp32; Kw <= 16; alpha [Cin] or null (no Snake); bias may be null. */
int kk_op_snac_conv_cout1(void* stream, int B, const void* x, int dtype, int ld, int L, int Cin, int Kw, int pad, const float* w_packed, int ldw,
                          const float* bias, const float* alpha, int tanh_out, float* out);

/* =====================================================================================================================
 * Row-mode polyphase FIR resampler (ABI minor 10): the sample-rate edge of CSM serving.  The reference resamples whole clips
 * with a Fourier scipy.signal.resample (sesame.py load_audio); a stream fed in arbitrary slices needs a causal filter whose bits do not
 * depend on the slicing.  For a row with ratio L / M (destination / source rate over their gcd), half = 10 max(L, M) and the 2 half + 1 taps
 *   h = firwin(2 half + 1, 1 / max(L, M), window = ("kaiser", 5.0)) L        (designed by the caller: mlx-audio_amd/resample.py design)
 * output n of a clip x[0..N) is
 *   y[n] = sum_j h[n M + half - j L] x[j],  x = 0 outside [0, N),  0 <= n < out_len(N) = ceil(N L / M)
 * which is scipy.signal.resample_poly(x, L, M) with its defaults.  While a stream is open and N samples were fed, the outputs below
 * ready(N) = max(0, (N L - 1 - half) / M + 1) (floor) are final; a flush emits the rest up to out_len(N) with zeros behind the clip.
 * Each output is ONE fmaf chain from 0.0f over its phase's T = ceil((2 half + 1) / L) taps in ascending input order, zeros multiplied like
 * samples, so an output's bits depend on its index and the clip alone: any slicing of the steps, any row, any neighbours give the same bits.
 *   kk_resampler_create: max_rows <= 64 rows, at most max_in_per_step new samples per row and step.
 *   kk_resampler_set_row: a new stream starts in `row` with zero history and zero counts.  max(L, M) <= 320.  taps: HOST fp32, phase-major
 *     [L][T], taps[p][t] = h[p + t L], zero where p + t L > 2 half; copied before the call returns.  Enqueues two copies and a memset.
 *   kk_resampler_step: x [max_rows][ldx] and y [max_rows][ldy] on the device (x 16-byte aligned, ldx % 4 == 0); n_in, flush and n_out are HOST
 *     arrays [max_rows].  A row with n_in == 0 and flush == 0 sits out: nothing of it is read (its x entries may hold NaN), nothing of it
 *     changes, n_out = 0.  Any other row consumes x[row][0 .. n_in) and writes its next n_out = ready(N) - emitted outputs (flush:
 *     out_len(N) - emitted) to y[row][0 .. n_out).  n_out is host integer arithmetic on a mirror of the device counts: no step synchronises.
 *     One launch for all rows; the carried state (the last T inputs, inputs consumed, outputs emitted) stays on the device.
 *   kk_resampler_block_outputs: the outputs one workgroup owns (tests place their edge lengths around it).
 *   kk_op_resample: a whole clip, stateless: x [N] and y [out_len(N)] on the device (x 16-byte aligned), taps on the HOST.  A one-row
 *     resampler is created, stepped once with flush and destroyed; synchronises `stream`.
 * All work is enqueued on the `stream` of the call: the caller passes the stream of the consumer (or producer) of y, which orders the two.
 * Refused on the host before any launch, with nothing changed: a row out of range, max(L, M) > 320, a T that does not fit L / M, n_in < 0,
 * n_in > max_in_per_step or > ldx, n_out > ldy, a row without a ratio, a step of a row after its flush, a misaligned x.
 * ===================================================================================================================== */
typedef struct kk_resampler kk_resampler;
int kk_resampler_create(int max_rows, int max_in_per_step, kk_resampler** out);
void kk_resampler_destroy(kk_resampler* r);
int kk_resampler_set_row(kk_resampler* r, void* stream, int row, int L, int M, const float* taps, int T);
int kk_resampler_step(kk_resampler* r, void* stream, const float* x, long long ldx, const int32_t* n_in, const int32_t* flush, float* y,
                      long long ldy, int32_t* n_out);
int kk_resampler_block_outputs(void);
int kk_op_resample(void* stream, const float* x, int N, int L, int M, const float* taps, int T, float* y);

/* =====================================================================================================================
 * PCM wire formats (ABI minor 11): what a phone line, a browser microphone and a playback device speak.  A sample is stored as
 *   KK_PCM_F32    4 bytes, the float itself
 *   KK_PCM_S16LE  2 bytes, little-endian int16 s:  x = s / 32768 (exact);  s = clamp(rint(x 32768), -32768, 32767), ties to even,
 *                 +-inf -> full scale, NaN -> 0
 *   KK_PCM_MULAW  1 byte, G.711 mu-law of s (decodes to +-32124);  KK_PCM_ALAW  1 byte, G.711 A-law of s (decodes to +-32256)
 * with the integer rules of Python's audioop at width 2 (lin2ulaw, ulaw2lin, lin2alaw, alaw2lin), computed with shifts and a count of
 * leading zeros, no table.  encode(decode(c)) == c for every int16, every A-law octet and every mu-law octet but 0x7F (negative zero -> 0xFF).
 *   kk_resampler_set_row_fmt: kk_resampler_set_row with the format the row's new samples are stored as and the format its outputs are stored
 *     as.  kk_resampler_set_row means f32 for both.
 *   kk_resampler_step_fmt: kk_resampler_step on BYTE buffers: x [max_rows][ldx_bytes] and y [max_rows][ldy_bytes], both 16-byte aligned with
 *     pitches that are multiples of 16.  n_in and n_out count SAMPLES of the row's own formats.  Samples are decoded as they are staged (the
 *     carried history stays fp32) and the outputs are encoded as they are stored: a row's outputs are encode(resample(decode(clip))) bit for
 *     bit, and an f32 -> f32 row gives the bits kk_resampler_step gives.  kk_resampler_step refuses a row whose formats are not both f32.
 *   kk_pcm_convert_rows: rows that need no ratio: y[row][i] = encode(decode(x[row][i])), i < n[row], any format to any format, stateless.
 *     in_fmt, out_fmt and n are HOST arrays [rows], rows <= 64; a row with n = 0 sits out and nothing of it is read.  One launch.
 *   kk_op_pcm_convert: one row x [n] -> y [n] (both 16-byte aligned), for tools and tests.  Neither entry synchronises.
 * Refused on the host before any launch, with nothing changed: an unknown format, a misaligned x or y, a pitch that is not a multiple of 16,
 * a row too short for its n_in, n_out or n in its own sample size.
 * ===================================================================================================================== */
enum { KK_PCM_F32 = 0, KK_PCM_S16LE = 1, KK_PCM_MULAW = 2, KK_PCM_ALAW = 3 };
int kk_resampler_set_row_fmt(kk_resampler* r, void* stream, int row, int L, int M, const float* taps, int T, int in_fmt, int out_fmt);
int kk_resampler_step_fmt(kk_resampler* r, void* stream, const void* x, long long ldx_bytes, const int32_t* n_in, const int32_t* flush, void* y,
                          long long ldy_bytes, int32_t* n_out);
int kk_pcm_convert_rows(void* stream, int rows, const void* x, long long ldx_bytes, const int32_t* in_fmt, void* y, long long ldy_bytes,
                        const int32_t* out_fmt, const int32_t* n);
int kk_op_pcm_convert(void* stream, const void* x, int in_fmt, void* y, int out_fmt, int n);

/* =====================================================================================================================
 * Row-mode voice-activity detector (ABI minor 12): endpointing and barge-in for the listening edge of CSM serving.  The
 * reference's energy rule and listener loop (mlx_audio/sts/voice_pipeline.py _is_silent, _listener; webrtcvad's model is not restated):
 * a frame of frame_len samples is speech iff its energy E = sum x^2 >= thr2n = float32(threshold^2 frame_len) -- rms >= threshold without
 * the square root and the division -- and, per row and in frame order,
 *   speech:  speaking = 1, silent = 0, last_speech = f, onset = f if there was none
 *   silence while speaking:  ++silent; silent > hang_frames: endpoint = f, and the row classifies nothing after it
 *   silence before any speech:  nothing
 * E is ONE wave's fixed order: lane l runs acc = fmaf(x[i], x[i], acc) from 0.0f over i = l, l + 64, ... ascending within the frame, and an
 * xor butterfly over the distances 32, 16, 8, 4, 2, 1 adds the 64 partial sums; E's bits depend on the frame's samples alone.  A NaN energy
 * compares false and reads as silence.
 *   kk_vad_create: max_rows <= 64 independent streams.
 *   kk_vad_set_row: a new stream starts in `row` with zero counts and no onset (one tiny launch on `stream`).  frame_len in [1, 4096],
 *     hang_frames >= 0, thr2n finite and >= 0 (computed by the caller in double precision, rounded once).
 *   kk_vad_step: x [max_rows][ldx] on the device; x[row][0 .. n_avail[row]) is the row's stream FROM ITS FIRST SAMPLE, the same buffer every
 *     step.  n_avail is a HOST array [max_rows].  The step classifies the whole frames classified <= f < n_avail / frame_len.  A row whose
 *     n_avail gives no new whole frame sits out, as does a row without a kk_vad_set_row and a row that has reached its endpoint: nothing
 *     of it is read (it may hold NaN), its state and status stay.  status [max_rows][4] int32 on the DEVICE: {classified, onset,
 *     last_speech, endpoint} per row, -1 for "none", written for the rows that took part.  energy: NULL, or [max_rows][lde] fp32 on the
 *     device: the E of the frames this step classified, energy[row][f - first new frame].  One launch, one workgroup per row; no
 *     synchronisation: the host mirrors the frame count with integers.
 *   kk_op_vad: a whole clip x [n] (device) on a one-row detector; status_host [4] on the HOST, energy_or_null [n / frame_len] on the device.
 *     Synchronises `stream`.  For tools and tests.
 * Refused on the host before any launch, with nothing changed: a row out of range, frame_len or hang_frames out of range, a negative,
 * infinite or NaN thr2n, an n_avail below the row's previous one or above ldx, an lde shorter than a row's new frames.
 * ===================================================================================================================== */
typedef struct kk_vad kk_vad;
int kk_vad_create(int max_rows, kk_vad** out);
void kk_vad_destroy(kk_vad* v);
int kk_vad_set_row(kk_vad* v, void* stream, int row, int frame_len, float thr2n, int hang_frames);
int kk_vad_step(kk_vad* v, void* stream, const float* x, long long ldx, const int32_t* n_avail, int32_t* status, float* energy, long long lde);
int kk_op_vad(void* stream, const float* x, int n, int frame_len, float thr2n, int hang_frames, int32_t status_host[4], float* energy_or_null);

/* =====================================================================================================================
 * Re-arming voice-activity detector over a ring (ABI minor 13): a microphone that stays open.  The rule, the energy and its
 * bits are kk_vad's; what differs is the coordinates and what happens behind an utterance.  A row's stream is numbered from 0 at
 * kk_vad_ring_set_row, in 64-bit positions everywhere (launch tables, device state, status), and sample p lives at x[row][p % ring_len],
 * frame_len <= ring_len <= ldx, so frame f = positions [f frame_len, (f + 1) frame_len) wraps at most once.  Only the address is taken
 * modulo the ring: E is bit-equal to kk_op_vad on the same stream laid out flat.  Per row and in frame order,
 *   speech:  speaking = 1, silent = 0, last_speech = f, onset = f if there was none
 *   silence while speaking:  ++silent; silent > hang_frames closes the utterance at endpoint = f (flags 0)
 *   otherwise, while speaking:  f - onset + 1 == max_frames closes it at endpoint = f with flags 1 ("forced")
 *   closing appends {onset, last_speech, endpoint, flags} to the row's log and re-arms (speaking = silent = 0, onset = last_speech = -1);
 *   the walk goes on with frame f + 1 in the same launch.  NaN energy reads as silence, inf as speech.
 * The log is a device ring of KK_VAD_LOG = 8 records per row: record k (counted from 0 at set_row) lives at log[row][k % 8].  The step's
 * acked[row] is the number of records the host has consumed; the walk stops in front of any frame while closed - acked == 8, and a later
 * step resumes from the device's own `classified` (the caller keeps those frames in the ring until a status shows them classified).
 *   kk_vad_ring_step: x [max_rows][ldx] fp32 on the device; n_avail and acked are HOST arrays [max_rows] of int64: the row's samples so far
 *     and its consumed records.  status [max_rows][4] int64 on the DEVICE: {classified, closed, onset, last_speech}, the last two of the open
 *     utterance, -1 for none; log [max_rows][8][4] int64 on the DEVICE.  Both are written by the rows that walked.  energy: NULL, or
 *     [max_rows][lde] fp32 on the device, frame f's E at energy[row][f % lde].  A row takes part when n_avail gives a new whole frame or
 *     acked has moved; a row without a set_row sits out and nothing of it is read.  One launch, one workgroup per row, no synchronisation.
 * Refused on the host before any launch, with nothing changed: a row out of range, frame_len outside [1, 4096], ring_len < frame_len or
 * > ldx, a negative hang_frames, max_frames < 1, a negative, infinite or NaN thr2n, an n_avail below the row's previous one, an n_avail -
 * ring_len above the first position of the oldest frame not yet handed to a step (unseen samples would have been overwritten), an acked
 * below its previous value or above the frames handed out before this step (a record takes a frame of its own).
 * ===================================================================================================================== */
#define KK_VAD_LOG 8
typedef struct kk_vad_ring kk_vad_ring;
int kk_vad_ring_create(int max_rows, kk_vad_ring** out);
void kk_vad_ring_destroy(kk_vad_ring* v);
int kk_vad_ring_set_row(kk_vad_ring* v, void* stream, int row, int frame_len, float thr2n, int hang_frames, long long max_frames, long long ring_len);
int kk_vad_ring_step(kk_vad_ring* v, void* stream, const float* x, long long ldx, const int64_t* n_avail, const int64_t* acked, int64_t* status,
                     int64_t* log, float* energy, long long lde);

/* =====================================================================================================================
 * Row-table ring copies (ABI minor 13): rows <= 64 rows in one launch, the table a launch argument.  pos, n and n_total are
 * HOST arrays [rows]; src, ring and dst are fp32 on the device with pitches lds, ldr, ldd in floats; ring_len <= ldr is every row's ring.
 *   kk_ring_write_rows: ring[b][(pos[b] + i) % ring_len] = src[b][i], i < n[b].  A row with n = 0 sits out.
 *   kk_ring_read_rows:  dst[b][i] = ring[b][(pos[b] + i) % ring_len], i < n[b], and 0.0f for n[b] <= i < n_total[b].  A row with
 *     n_total = 0 is not touched.
 * 16-byte accesses where both sides are aligned and the run does not wrap, element by element otherwise: a copy either way.
 * Refused on the host before any launch: rows outside [1, 64], n > ring_len, n > n_total, a negative count or position, a row longer than
 * its pitch (n > lds, n_total > ldd, ring_len > ldr).  Neither entry synchronises.
 * ===================================================================================================================== */
int kk_ring_write_rows(void* stream, int rows, const float* src, long long lds, float* ring, long long ldr, long long ring_len, const int64_t* pos,
                       const int32_t* n);
int kk_ring_read_rows(void* stream, int rows, const float* ring, long long ldr, long long ring_len, float* dst, long long ldd, const int64_t* pos,
                      const int32_t* n, const int32_t* n_total);

/* =====================================================================================================================
 * CSM-1B frame generator (rows C1-C3): SesameModel.generate_frame, mlx_audio/tts/models/sesame/sesame.py:349-395, with the
 * Llama stacks of mlx_lm (LlamaModel + the reference's Attention / Llama3ScaledRoPE, attention.py).  fp32 arithmetic; in bf16 weight
 * mode the single-token steps run as five launches per layer on the fused GEMV (no split-K partials, norm / SwiGLU / residual fused).
 * ===================================================================================================================== */
typedef struct kk_csm kk_csm;
typedef struct kk_llama_args { /* sesame.py:225-273 */
  int32_t num_layers, num_heads, num_kv_heads, head_dim, hidden, intermediate;
  float rope_theta, rope_factor, rms_eps; /* 500000, 32 (llama3 scaling: low 1, high 4, old context 8192), 1e-5 */
} kk_llama_args;
typedef struct kk_csm_config {
  int32_t text_vocab_size, audio_vocab_size, audio_num_codebooks, max_seq_len; /* 128256, 2051, 32, 2048 */
  kk_llama_args backbone, decoder;                                              /* llama-1B, llama-100M */
} kk_csm_config;

int kk_csm_create(const kk_csm_config* cfg, kk_csm** out);
void kk_csm_destroy(kk_csm* m);
/* MLX-side names: {backbone,decoder}.layers.N.{self_attn.{q,k,v,o}_proj,mlp.{gate,up,down}_proj,input_layernorm,
 * post_attention_layernorm}.weight, {backbone,decoder}.norm.weight, text_embeddings.weight, audio_embeddings.weight,
 * projection.weight, codebook0_head.weight, audio_head [n_cb-1][decoder_dim][audio_vocab]; host fp32 */
int kk_csm_load_tensor(kk_csm* m, const char* name, const int64_t* shape, int ndim, const float* data);
/* weight storage of the Linear layers: KK_DTYPE_F32 (default) or KK_DTYPE_BF16 -- matrices rounded to bf16 once (lossless for the
 * bf16 checkpoints load_model keeps in their own dtype, tts/utils.py:217-262), 2-byte weight stream in the single-token steps with
 * SwiGLU applied while the down projection stages its input; activations, accumulation, KV cache, logits stay fp32.  Before finalize. */
int kk_csm_set_weight_dtype(kk_csm* m, int dtype);
/* A quantised nn.Linear / nn.Embedding of an MLX affine-quantised checkpoint (tts/utils.py:241-260; ABI minor 1): shape [O, I] of the
 * DEquantised matrix, words uint32 [O][I bits / 32] (value j of a word in bits [j bits, (j + 1) bits)), scales / biases fp32 [O][I / group_size];
 * w = scales * q + biases per group.  Host data, copied; before finalize; a name loaded both ways keeps the later call.  bits 2, 4 or 8.
 * kk_csm_finalize then decides ONCE for the whole model: PACKED storage -- every Linear of the frame step (q|k|v, o, gate|up, down of both
 * stacks, projection, codebook0_head) stays quantised in device memory and is decoded to bf16 inside the matrix-core kernels, as
 * bf16_rne(fp32(q) * scale + bias) (fp32 multiply, fp32 add: the bf16 rounding of the dequantised matrix, so the frames carry the bits of bf16
 * weight mode on the dequantised checkpoint), with no fp32 and no bf16 copy -- if all of them arrived quantised with bits 4 or 8, one (bits,
 * group_size) per stacked matrix, group_size a multiple of 32 that divides I, and every one gets a fragment pack (kk_csm_frag_choice); otherwise
 * the whole checkpoint is dequantised on the host and runs in bf16 weight mode.  Embedding tables are always dequantised into their fp32 tables. */
int kk_csm_load_quantized(kk_csm* m, const char* name, const int64_t* shape, const uint32_t* words, const float* scales, const float* biases,
                          int group_size, int bits);
/* what kk_csm_finalize decided: one of KK_CSM_WEIGHTS_F32 / BF16 / Q8 / Q4, | KK_CSM_WEIGHTS_MIXED (packed, some Linears 8-bit and some 4-bit),
 * | KK_CSM_WEIGHTS_DEQUANTIZED (a quantised checkpoint that fell back to host dequantisation; kk_csm_weight_fallback_reason says why); < 0: error */
#define KK_CSM_WEIGHTS_F32 0
#define KK_CSM_WEIGHTS_BF16 1
#define KK_CSM_WEIGHTS_Q8 2
#define KK_CSM_WEIGHTS_Q4 3
#define KK_CSM_WEIGHTS_MIXED 0x100
#define KK_CSM_WEIGHTS_DEQUANTIZED 0x200
int kk_csm_weight_format(const kk_csm* m);
const char* kk_csm_weight_fallback_reason(const kk_csm* m);
/* device bytes held for the Linear matrices (fp32 copies, bf16 / quantised fragment packs, pairs) and for all weights (+ norms, embedding
 * tables, RoPE tables, the projection table) */
int kk_csm_weight_bytes(const kk_csm* m, size_t* linear_bytes, size_t* total_bytes);
int kk_csm_finalize(kk_csm* m, void* stream);
/* A second generator on the SAME device weights (immutable after kk_csm_finalize): own KV caches, positions, logits and graph cache, for another
   stream / thread in flight; `m` must outlive it; kk_csm_setup_caches before its first frame.  (The reference's SesameModel owns its caches,
   sesame.py:320-333, and is single threaded.) */
int kk_csm_share(const kk_csm* m, kk_csm** out);
int kk_csm_setup_caches(kk_csm* m, int max_batch); /* SesameModel.setup_caches (sesame.py:320-333): library-owned KV caches */
int kk_csm_reset_caches(kk_csm* m);                /* sesame.py:338-345: positions restart at 0 */
int kk_csm_position(const kk_csm* m);              /* tokens in the backbone cache */
/* Ragged prompts in one batch (the reference's generate is batch 1, sesame.py:689-817): the prompts are LEFT-padded to the longest one
 * (padding frames: all-zero mask) and pad[b] (HOST array, B entries) says how many padding frames item b has.  Item b's token in cache
 * slot p then sits at position p - pad[b] and attends to slots >= pad[b] only: bit-identical to running the item alone.  Empty cache only. */
int kk_csm_set_padding(kk_csm* m, int B, const int32_t* pad_host);
size_t kk_csm_workspace_bytes(kk_csm* m, int B, int S);
/* One audio frame.  tokens [B][S][n_cb+1] int32 and tokens_mask (same shape, float 0/1) on the device; the S new positions continue
 * the backbone cache (a block of S > 1 must start an empty cache, as index_causal_mask implies, sesame.py:41-48).  Sampling:
 * temperature == 0 or uniforms == NULL -> argmax (make_sampler's rule for temp 0); otherwise inverse CDF over the top_k logits
 * (top_k 0 / -1: the whole vocabulary; see kk_csm_sampler) of softmax(logit / temperature) in descending order with the injected
 * uniforms [B][n_cb] -- the distribution of make_sampler(temp, top_k) with a reproducible draw.  codes_out [B][n_cb] int32. */
int kk_csm_generate_frame(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, float temperature, int top_k,
                          const float* uniforms, void* workspace, size_t workspace_bytes, int32_t* codes_out);
/* The sampler of a frame: mlx_lm's make_sampler(temp, top_p, min_p, min_tokens_to_keep, top_k) as sesame.py:696,719 takes it.  mlx_lm is not
 * part of the reference tree: the rule below is written from upstream knowledge and parity with mlx_lm is UNPINNED.
 *   l[0..V) one row of fp32 logits (a NaN reads as -inf); order = indices by (logit descending, index ascending); p = softmax(l) over the
 *   WHOLE vocabulary at temperature 1 (the filters see untempered probabilities; the temperature acts in the draw only).  Every filter keeps a
 *   prefix of `order`, the kept set is the shortest:
 *     n_k = top_k if 0 < top_k < V, else V (0 and -1 switch the filter off; no clamp at 64);
 *     n_p: with 0 < top_p < 1, order[j] is kept iff sum(p[order[:j]]) < top_p (the first token always); else V;
 *     n_m: with min_p > 0, the tokens with p >= min_p p[order[0]], never fewer than min_tokens_to_keep; else V;
 *     n = min(n_k, n_p, n_m); weights w[j] = exp((l[order[j]] - l[order[0]]) / temperature) for j < n, running sums c, target = u c[n-1],
 *     the pick is order[j] for the first j with c[j] >= target (the last kept token if none).
 *   temperature == 0, or no uniform source: arg-max, lower index on ties.  A pick is always in [0, V).
 * Uniforms: the injected array has priority.  Without it and with use_device_rng, Philox4x32-10 in the sampling kernels:
 *   philox4(seed, (uint64) stream_id << 32 | pos, code book) -> u = ((out[0] >> 8) + 0.5) 2^-24, in (0, 1); pos = the item's own position of the
 *   frame being generated (cache slot minus its padding), stream_id = stream_ids[b] or b.  Nothing in the counter depends on the batch layout.
 * With top_p and min_p off and 0 < top_k <= 64 the kernel and the picks are those of kk_csm_generate_frame before this struct existed. */
typedef struct kk_csm_sampler {
  float temperature;
  int32_t top_k;
  float top_p, min_p;
  int32_t min_tokens_to_keep;
  uint64_t seed;
  int32_t use_device_rng;
} kk_csm_sampler;
/* kk_csm_generate_frame with the whole sampler; kk_csm_generate_frame is this call with {temperature, top_k, 0, 0, 1, 0, 0} and no stream ids.
 * stream_ids: device int32 [B] or NULL (read by the kernels at every frame, replayed graphs included).  The seed is copied to device memory
 * when it changes, so a new seed replays the same graph; every other sampler field and the stream_ids pointer key the graph. */
int kk_csm_generate_frame_ex(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, const kk_csm_sampler* sampler,
                             const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out);
/* Per-row sampler settings: a device table with one 32-byte entry per cache row, {temperature, top_k, top_p, min_p, min_tokens_to_keep, pad, seed},
 * read by the sampling kernel of the row's workgroup instead of launch arguments.  kk_csm_setup_caches and kk_csm_reset_caches_parked zero it; a
 * zero entry has temperature 0: arg-max, so a parked or never-set row still yields codes in [0, V).
 *   kk_csm_set_row_sampler: validates the sampler (the rule of every entry above) and the row on the host, then writes the entry in stream order
 *     (the values travel as launch arguments: `sampler` need not outlive the call).  `seed` is stored and read only by launches that draw on the
 *     device; use_device_rng is a property of the frame call, not of the entry.
 *   kk_csm_generate_frame_rows: kk_csm_generate_frame_ex with the sampler of item b read from table row b -- the same launches, and row b's codes
 *     are, bit for bit, those of the launch-argument kernels with the entry's values.  Any S the _ex call accepts.  uniforms [B][n_cb] have priority;
 *     without them and with use_device_rng each row draws Philox on ITS entry's seed (stream id, position and code book as before); without either,
 *     arg-max.  Graph mode: the captured step is keyed by this mode, B, the pointers and the uniform source, never by what the table holds -- a
 *     kk_csm_set_row_sampler between two replays takes effect in the next replay without a new capture.
 * kk_csm_admit / kk_csm_admit_prefixed are unchanged: they take the request's sampler for their B = 1 block. */
int kk_csm_set_row_sampler(kk_csm* m, void* stream, int row, const kk_csm_sampler* sampler);
int kk_csm_generate_frame_rows(kk_csm* m, void* stream, int B, int S, const int32_t* tokens, const float* tokens_mask, int use_device_rng,
                               const float* uniforms, const int32_t* stream_ids, void* workspace, size_t workspace_bytes, int32_t* codes_out);
/* Continuous batching: streams enter and leave a RUNNING batch (after kk_csm_setup_caches(max_batch); none of these changes what the entries
 * above do).  All rows share the slot counter P (kk_csm_position); row b's tokens live in slots [pad[b], P) at position slot - pad[b].
 *   kk_csm_park_row: the row is retired -- pad[row] = max_seq_len.  From the next frame on its attention sees no key (zero output) and appends
 *     nothing; it still rides through the frame step, its codes are unspecified but in [0, V), and nothing it does reaches another row.
 *   kk_csm_reset_caches_parked: kk_csm_reset_caches (P = 0) with EVERY row parked, the start of a serving session.  The classic reset leaves
 *     every row live (pad 0), as before.
 *   kk_csm_admit: the prompt frame of ONE new stream (tokens / tokens_mask [S][n_cb+1] on the device) into the parked row `row` while other rows
 *     are live.  Needs S <= P.  Sets pad[row] = P - S, runs the prompt block on that row alone at slots [P - S, P) -- the kernels and B = 1 shapes
 *     of kk_csm_generate_frame_ex(B = 1, S) on an empty cache, so codes_out [n_cb] carries that call's bits --, and does NOT advance P: from the
 *     next frame on the row is an ordinary row of the single-token step.  uniforms [n_cb] or NULL; the device RNG draws at (stream_id, position S).
 *     Never captured into a graph; the captured frame step of the other rows stays valid.
 *   kk_csm_shift_caches: moves the window [pad[b], P) of every live row by `delta` slots (either sign, overlap allowed) in every layer's K and V and
 *     adds delta to P and to every live pad[b].  Keys are stored rotated by the stream's OWN position, which does not change, so the move is exact.
 *     Down by min(pad[live]) when P reaches max_seq_len; up by S - P before admitting a prompt longer than P.  Fails, changing nothing, if P or a
 *     live window would leave [0, max_seq_len).  workspace is unused (may be NULL).
 *   kk_csm_row_state: pad_out [max_batch] (HOST; max_seq_len = parked) and P, as the next frame will see them.
 * Every refusal (live row, row out of range, S > P, a window leaving the cache, no caches) is decided on the host before any launch. */
int kk_csm_admit(kk_csm* m, void* stream, int row, int S, const int32_t* tokens, const float* tokens_mask, const kk_csm_sampler* sampler,
                 const float* uniforms, int32_t stream_id, void* workspace, size_t workspace_bytes, int32_t* codes_out);
int kk_csm_park_row(kk_csm* m, int row);
int kk_csm_reset_caches_parked(kk_csm* m);
int kk_csm_shift_caches(kk_csm* m, void* stream, int delta, void* workspace, size_t workspace_bytes);
int kk_csm_row_state(const kk_csm* m, int32_t* pad_out, int32_t* position);
/* A shared voice prefix: the backbone K / V of `n` prompt positions that many streams start with (a speaker's reference segment), computed once
 * and copied under every stream admitted on top of it.  A key is stored rotated by its stream's OWN position, so the K / V of positions 0 .. n-1
 * depend on neither the cache row, nor the slot, nor what follows them.
 *   kk_csm_prefix_create: runs the backbone prompt block of ONE stream (tokens / tokens_mask [S][n_cb+1] on the device) at positions 0 .. S-1
 *     into a buffer of its own, [layer][K|V][S][kv_heads * head_dim] fp32 -- no depth decoder, no sampler.  It touches no cache row, neither P nor
 *     pad, is never captured and leaves captured frame steps valid: legal while a batch runs (pass a workspace that no captured step uses, of
 *     kk_csm_workspace_bytes(m, 1, S) bytes).  The object is immutable and records the weight set it was computed with; generators made by
 *     kk_csm_share from the same weights may all use it.  It needs no caches.
 *   kk_csm_prefix_length / kk_csm_prefix_bytes: n / the buffer's bytes (-1 / 0 for a null or destroyed prefix).
 *   kk_csm_prefix_read: the buffer, device to device (tests: a prefix does not change under the streams that use it).
 *   kk_csm_admit_prefixed: kk_csm_admit for a stream whose prompt is the prefix followed by the S >= 1 frames of `tokens`.  Needs n + S <= P and a
 *     parked row.  Sets pad[row] = P - n - S, copies the prefix into the row's slots [P - n - S, P - S) (one launch for all layers' K and V), runs
 *     the suffix block at slots [P - S, P) -- positions n .. n+S-1 --, then the depth decoder and the sampler as kk_csm_admit does; the device RNG
 *     draws at (stream_id, position n + S).  P does not move.  Both entries run their blocks through the PROMPT kernels whatever the row count
 *     (a block of one or two rows is not sent to the single-token kernels), so codes_out and the row's K / V carry, bit for bit, what
 *     kk_csm_generate_frame_ex(B = 1, n + S) computes on the whole prompt from an empty cache.
 *   kk_csm_prefix_capture (ABI minor 7): the first n positions of LIVE row `row` -- slots [pad[row], pad[row] + n) of K and V in every backbone layer --
 *     as a new immutable prefix of the same layout, tied to the weight set as kk_csm_prefix_create ties it.  One copy launch; it reads nothing but
 *     that row's window and writes nothing but its own buffer: P, pad and captured frame steps are untouched, so it is legal between two frames of
 *     a running batch.  Positions that a single-token step appended carry that step's bits, not a prompt block's; they are the same bits whatever
 *     row, slot and batch the stream ran in.  Refused: no caches, row out of range, a parked row, n < 1, n > P - pad[row], kv_heads * head_dim % 4.
 *   kk_csm_admit_transfer (ABI minor 8): an admission prefilled on ANOTHER generator of the same weights (kk_csm_share) enters this one.  `src_row` of
 *     `src` is a live row whose window [pad_s, P_s) holds the L = P_s - pad_s positions of a finished kk_csm_admit / kk_csm_admit_prefixed; `row` of
 *     `m` is parked.  Sets pad[row] = P - L and copies the window into slots [P - L, P) of `row` in every backbone layer's K and V: one copy launch,
 *     no prompt block, no depth decoder, no sampler.  P, the other rows, the frame-step graph and its key are untouched (legal between two replays);
 *     `src_row` stays live, the caller parks it.  The entry orders the two streams itself: `stream` waits for what `src_stream` holds at the call,
 *     and `src_stream` waits for the copy (events owned by `m`; no allocation and no synchronisation on this path).  Refused on the host, with
 *     nothing changed: m == src, no caches on either side, a row out of range, `row` live, `src_row` parked, L < 1, L > P (kk_csm_shift_caches by
 *     L - P first), different weight sets or K / V geometry, kv_heads * head_dim not a multiple of 4.
 * Refusals (live row, row out of range, n + S > P, a prefix of another weight set, a null or destroyed prefix, workspace too small) are decided
 * on the host before any launch. */
typedef struct kk_csm_prefix kk_csm_prefix;
int kk_csm_prefix_create(kk_csm* m, void* stream, int S, const int32_t* tokens, const float* tokens_mask, void* workspace, size_t workspace_bytes,
                         kk_csm_prefix** out);
int kk_csm_prefix_length(const kk_csm_prefix* p);
size_t kk_csm_prefix_bytes(const kk_csm_prefix* p);
int kk_csm_prefix_read(const kk_csm_prefix* p, void* stream, float* dst, size_t dst_bytes);
void kk_csm_prefix_destroy(kk_csm_prefix* p);
int kk_csm_prefix_capture(kk_csm* m, void* stream, int row, int n, kk_csm_prefix** out);
int kk_csm_admit_transfer(kk_csm* m, void* stream, int row, kk_csm* src, void* src_stream, int src_row);
int kk_csm_admit_prefixed(kk_csm* m, void* stream, int row, const kk_csm_prefix* prefix, int S, const int32_t* tokens, const float* tokens_mask,
                          const kk_csm_sampler* sampler, const float* uniforms, int32_t stream_id, void* workspace, size_t workspace_bytes,
                          int32_t* codes_out);
/* graph replay of the single-token frame step: the third call with identical pointers / B / sampler settings and every later one is ONE
 * hipGraphLaunch (the backbone position is a device counter, so the captured step is position-independent); results are unchanged */
int kk_csm_set_graph_mode(kk_csm* m, int on);
int kk_csm_debug_logits(kk_csm* m, void* stream, int B, float* dst); /* logits of the last frame, [n_cb][B][audio_vocab] */
/* In-kernel wall-clock marks (100 MHz counter) of the single-token step's instrumented kernels, 8 uint64 per launch in launch order:
   class id, earliest workgroup start, latest workgroup end, workgroup 0 after its input loads, then workgroup 0's own start, shader-clock
   count at start, end, shader-clock count at end (core clock = cycles / wall x 100 MHz).  buf: device memory for `capacity`
   launches, the caller fills words 1 with ~0 and 2 with 0 before a frame; NULL switches the marks off.  Process-wide, debugging only
   (tools/csm_timeline.py). */
int kk_csm_debug_timestamps(unsigned long long* buf, int capacity);
/* the sampler of generate_frame on its own (mlx_lm make_sampler(temp, top_k), sesame.py:335-336,719): logits [B][V] -> codes [B];
 * uniforms [B] or NULL (argmax).  Radix select of the top_k set + one-wave sort; V <= 8192. */
int kk_op_csm_sample(void* stream, int B, int V, const float* logits, float temperature, int top_k, const float* uniforms, int32_t* codes_out);
/* kk_op_csm_sample with the whole kk_csm_sampler, through the launcher the frame uses: uniforms [B] (priority) or, with use_device_rng, Philox on
 * (sampler->seed, stream_ids[b] or b, pos[b] or 0, code book 0); stream_ids / pos: device int32 [B] or NULL.  Synchronises when it draws on the device. */
int kk_op_csm_sample_ex(void* stream, int B, int V, const float* logits, const kk_csm_sampler* sampler, const float* uniforms, const int32_t* stream_ids,
                        const int32_t* pos, int32_t* codes_out);
/* kk_op_csm_sample_ex with one sampler PER ROW (samplers: HOST array [B]) through the launcher kk_csm_generate_frame_rows uses: a temporary device
 * table is uploaded, one launch serves all rows, then it synchronises and frees the table.  Row b's pick is that of kk_op_csm_sample_ex on row b alone
 * with samplers[b].  use_device_rng must agree across the entries (it is a property of the launch); each row draws on its own seed. */
int kk_op_csm_sample_rows(void* stream, int B, int V, const float* logits, const kk_csm_sampler* samplers, const float* uniforms,
                          const int32_t* stream_ids, const int32_t* pos, int32_t* codes_out);
/* the uniforms the sampling kernels draw: out [B][n_cb] (device) for (seed, stream_ids[b] or b, pos[b] or 0, code book 0..n_cb-1).  Synchronises. */
int kk_op_csm_uniforms(void* stream, int B, int n_cb, uint64_t seed, const int32_t* stream_ids, const int32_t* pos, float* out);
/* The kernels of the frame step on their own (tests), each through the launcher the frame runs.  Fragment pack of the bf16 weights (host):
 * kk_csm_frag_choice gives the split-K slices and 16-column sub-blocks per block the generator picks for a K x N matrix (nsub = 0: no pack;
 * split_ok: the matrix is a down projection, the one launched split-K); kk_csm_frag_pack lays w [K][N] fp32 out as bf16 (round to nearest
 * even) [ceil(N / (16 nsub))][K / 32][nsub][64][8], lane L of chunk c, sub-block s = k 32 c + 8 (L / 16) + j, column 16 s + L % 16. */
int kk_csm_frag_choice(int K, int N, int split_ok, int32_t* ks, int32_t* nsub);
int kk_csm_frag_pack(const float* w, int K, int N, int nsub, uint16_t* out);
/* Quantised fragment pack (host) of one nn.Linear triplet, words [N][K bits / 32], scales / biases [N][K / group_size] (bits 4 or 8, group_size a
 * multiple of 32 dividing K): q_out = the integers in the fragment order above, a lane's 8 values in 8 bytes (8-bit) or 4 bytes (4-bit), value j in
 * bits [j bits, (j + 1) bits); pairs_out = float2 (scale, bias) [ceil(N / (16 nsub))][K / group_size][nsub][16 columns].  Padding columns: all zero
 * (they decode to +0).  kk_csm_qfrag_bytes: K Npad bits / 8 and Npad (K / group_size) 8 bytes, Npad = N rounded up to 16 nsub. */
int kk_csm_qfrag_bytes(int K, int N, int nsub, int group_size, int bits, size_t* q_bytes, size_t* pair_bytes);
int kk_csm_qfrag_pack(const uint32_t* words, const float* scales, const float* biases, int K, int N, int nsub, int group_size, int bits, void* q_out,
                      float* pairs_out);
/* Single-token GEMV on the matrix cores, out[m] = prologue(x[m]) W (+ res[m]): pro 0 plain, 1 RMSNorm with nw / eps (codes: rows gathered from
 * emb, also written to gather_out), 2 silu(gate) * up of [gate | up] rows, 3 every `rows`-th row from emb by code (items of 1 or 2 rows); epi 0
 * store, 1 + res; ks > 1 (epi 2): split-K, out[M][N] += the sum of the slices (part: ks M N floats).  Device pointers, row pitches in floats. */
int kk_op_csm_gemv(void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const void* w_frag, const float* x, long long xrs,
                   const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb, float* gather_out,
                   const float* res, long long rrs, float* out, long long ors, float* part);
/* kk_op_csm_gemv on a quantised fragment pack + pairs (device): bit-identical to kk_op_csm_gemv on the bf16 pack of the dequantised matrix */
int kk_op_csm_gemv_q(void* stream, int pro, int epi, int ks, int nsub, int K, int N, int M, const void* q_frag, const void* pairs, int group_size, int bits,
                     const float* x, long long xrs, const float* nw, float eps, const int32_t* codes, int cstride, int cb, int V, int rows, const float* emb,
                     float* gather_out, const float* res, long long rrs, float* out, long long ors, float* part);
int kk_op_csm_gemm_prompt_q(void* stream, int K, int N, int M, int nsub, const void* q_frag, const void* pairs, int group_size, int bits, const float* x,
                            long long xrs, const float* res, long long rrs, float* out, long long ors);
/* the prompt block's GEMM: out[m] = x[m] W (+ res[m]) on a fragment pack */
int kk_op_csm_gemm_prompt(void* stream, int K, int N, int M, int nsub, const void* w_frag, const float* x, long long xrs, const float* res,
                          long long rrs, float* out, long long ors);
/* fp32-weight skinny GEMM of the single-token steps: out[M][N] = x[M][K] w[K][ldw] (+ res); scratch: K slices x 16 x N floats */
int kk_op_csm_linear_skinny(void* stream, int K, int N, int M, const float* w, int ldw, const float* x, const float* res, float* out, float* scratch,
                            size_t scratch_floats);
/* one new position per item: qkv [B][(H + 2 KV) hd], caches [B][max_pos][KV hd], rope [max_pos][hd / 2][2] cos | sin, pad [B] or NULL;
 * RoPE + append at slot `offset`, causal GQA attention over slots >= pad[b] -> out [B][H hd].  form 0: the step's choice, 1 short-cache
 * kernel (max_pos <= 64), 2 long-cache kernel + merge of its key splits (part: 8 B H (hd + 2) floats), 3 the general cache kernel */
int kk_op_csm_attn_single(void* stream, int form, int B, int H, int KV, int hd, const float* qkv, float* kc, float* vc, int max_pos, int offset,
                          const float* rope, const int32_t* pad, float* out, float* part);
/* a block of S new positions per item: RoPE (q in place) + append at slots offset .. offset + S - 1, then causal attention -> out [B][S][H hd] */
int kk_op_csm_attn_prompt(void* stream, int B, int S, int H, int KV, int hd, float* qkv, float* kc, float* vc, int max_pos, int offset, const float* rope,
                          const int32_t* pad, float* out);
/* the block forms Mimi's streaming transformer runs (no causal mask inside the block; ctx >= 0: only the last ctx cached keys + the block):
 * row_pos == NULL: RoPE + append at `offset` for every item, then the attention (kk_launch_rope_append + kk_launch_attn_cache);
 * otherwise item b sits at row_pos[b] and takes part only if active[b] != 0 (both device, [B]; `offset` unused): the per-row forms */
int kk_op_attn_cache_block(void* stream, int B, int S, int H, int KV, int hd, float* qkv, float* kc, float* vc, int max_pos, int offset,
                           const int32_t* row_pos, const int32_t* active, const float* rope, int ctx, float* out);

/* =====================================================================================================================
 * Whisper, audio side: log_mel_spectrogram (mlx_audio/stt/models/whisper/audio.py:41-82) and AudioEncoder / Model.embed_audio
 * (whisper.py:171-199, 295).  Device pointers unless stated, work enqueued on `stream`, no device-to-host synchronisation, 0 = OK.
 * ===================================================================================================================== */
/* audio.py:70-82 with stft and hanning of mlx_audio/utils.py:11-14: per row b of x [B][ldx] fp32 at 16 kHz with n[b] samples (n: device int32
 * [B]; the caller has checked n[b] + padding >= 201): `padding` zeros appended, 200 samples of reflect padding at both ends, frames of 400 at hop 160
 * under the symmetric Hann window, the 201-bin power spectrum, the last frame dropped (F[b] = (n[b] + padding) / 160 frames), the n_mels x 201
 * filter bank, log10(max(., 1e-10)), max(., row maximum - 8), (. + 4) / 4.  window [400], cos_sin [2][400] (cos | sin of 2 pi j / 400) and
 * fbT [201][n_mels] are the caller's fp32 tables, made in float64 on the host.  partial: scratch, B * F_rows floats.  out fp32 [B][F_rows][n_mels],
 * rows past F[b] written as zeros.  n_mels 80 or 128.  A row's bits depend on that row's samples alone. */
int kk_op_log_mel(void* stream, int B, const float* x, long long ldx, const int32_t* n, int padding, int n_mels, const float* window,
                  const float* cos_sin, const float* fbT, float* partial, float* out, int F_rows);
/* MultiHeadAttention.qkv_attention without a mask (whisper.py:123-137) for heads of 64 channels over a long sequence: qkv bf16 [B][T_rows][ld],
 * q | k | v at channels 0, heads * 64 and 2 * heads * 64 (ld >= 3 * heads * 64, ld % 8 == 0); out bf16 [B][T_rows][ldo] (ldo >= heads * 64, ldo % 4 == 0).
 * softmax(q k^T 64^-0.5) v over the first T rows (the reference's 64^-0.25 on each side is the same product); rows >= T are neither read as keys
 * nor written.  An item's bits do not depend on B. */
int kk_op_attention_long(void* stream, int B, const void* qkv, int ld, int T_rows, int T, int heads, void* out, int ldo);
/* The windows of a transcription round, cut out of whole-file spectrograms (whisper.py:641-644: mel[seek : seek + size], then pad_or_trim to W):
 * row r copies frames first[r] .. first[r] + size[r] - 1 of src[r] (DEVICE fp32 [frames[r]][n_mels], 16-byte aligned; the rows may lie in different
 * allocations) to out[r][0 .. size[r]) and writes zeros to out[r][size[r] .. W).  src, frames, first and size are HOST arrays of R entries that go to
 * the kernel by value: 1 <= R <= KK_WHISPER_MAX_ROWS, 0 <= size[r] <= W, first[r] >= 0, first[r] + size[r] <= frames[r] (refused otherwise before
 * anything is launched; src[r] may be null only where size[r] = 0).  out DEVICE fp32 [R][W][n_mels], 16-byte aligned.  n_mels 80 or 128.  One launch,
 * 16-byte loads and stores, no arithmetic. */
int kk_op_mel_windows(void* stream, int R, const float* const* src, const int32_t* frames, const int32_t* first, const int32_t* size, int W, int n_mels,
                      float* out);
/* Spans of sample buffers as Whisper windows (ABI minor 27).  Row r is n[r] >= 1 fp32 samples at the source rate: elements
 * pos[r] .. pos[r] + n[r] - 1 of the flat buffer buf[r] (ring_len[r] = 0), or samples (pos[r] + i) % ring_len[r] of a ring (n[r] <= ring_len[r]);
 * buf_len[r] is the buffer's element count.  out[r] is, bit for bit, the first W frames of kk_op_log_mel with padding = 160 W over
 * kk_op_resample(span, L, M) (L == M: over the span itself): the resampler's fmaf chain, the frame arithmetic and the row maximum over ALL frames
 * of the padded clip are the ones of those two entry points.  Nothing outside a span is read.  buf, buf_len, ring_len, pos and n are HOST arrays of
 * R entries that go to the kernel by value, 1 <= R <= KK_WHISPER_MAX_ROWS; a row whose ceil(n L / M) exceeds 160 W, a span outside its buffer and a
 * ratio whose frame does not fit the workgroup's LDS (served: L (T | 1) <= 512 and 399 M / L + T + 2 <= 1536, which covers 8, 12, 24, 32 and
 * 48 kHz) are refused before anything is launched.  tab: DEVICE fp32 [L][T], the phase table kk_resampler_set_row takes (unused when L == M);
 * window, cos_sin, fbT as for kk_op_log_mel.  partial: scratch, R * (W + 2) floats.  out DEVICE fp32 [R][W][n_mels].  W >= 3.  Two launches. */
int kk_op_log_mel_spans(void* stream, int R, const float* const* buf, const int64_t* buf_len, const int32_t* ring_len, const int64_t* pos,
                        const int32_t* n, int W, int L, int M, const float* tab, int T, int n_mels, const float* window, const float* cos_sin,
                        const float* fbT, float* partial, float* out);

typedef struct kk_whisper kk_whisper;
/* the audio fields of ModelDimensions (whisper.py:67-78); n_audio_state / n_audio_head must be 64, n_mels 80 or 128 */
typedef struct kk_whisper_config {
  int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
} kk_whisper_config;
int kk_whisper_create(const kk_whisper_config* cfg, kk_whisper** out);
void kk_whisper_destroy(kk_whisper* m);
/* encoder.* parameters by their MLX checkpoint names (whisper.py:171-187, 90-97, 140-155), host fp32, MLX layouts: conv weights [O][K][I],
 * Linear weights [out][in].  attn.key has no bias. */
int kk_whisper_load_tensor(kk_whisper* m, const char* name, const int64_t* shape, int ndim, const float* data);
/* rounds every matrix to bf16 (nearest even), packs and uploads; makes the sinusoidal positions (whisper.py:81-87) in fp32.  Fails naming a
 * missing or misshapen parameter.  Synchronises `stream`. */
int kk_whisper_finalize(kk_whisper* m, void* stream);
size_t kk_whisper_encode_workspace_bytes(const kk_whisper* m, int B);
/* AudioEncoder.__call__ (whisper.py:189-199): mel fp32 [B][2 * n_audio_ctx][n_mels] -> out fp32 [B][n_audio_ctx][n_audio_state] */
int kk_whisper_encode(kk_whisper* m, void* stream, int B, const float* mel, void* workspace, size_t workspace_bytes, float* out);

/* =====================================================================================================================
 * Whisper, text side: TextDecoder (whisper.py:202-248) and the token selection of decoding.py:255-395 (csrc/kk_whisper_text.hip).
 * Device pointers unless stated, work enqueued on `stream`, 0 = OK.  A row's bits never depend on how many rows a call carries or on what
 * the other rows hold.
 * ===================================================================================================================== */
/* One query row per r against a bf16 K/V store, heads of 64 channels: q fp32 [R][heads * 64]; kv bf16 [items][T_rows][ld] with the keys at
 * channel k_off and the values at v_off (multiples of 8, like ld); row r attends to the first len[r] keys of item item[r] (device int32 [R]);
 * out fp32 [R][heads * 64] = softmax(q k^T 64^-0.5) v in fp32.  Keys at or past len[r] and rows >= T_rows are not read.  scratch:
 * kk_op_whisper_attn_rows_scratch_bytes(R, heads, T_rows), 16-byte aligned.  This entry reads item / len back (it synchronises `stream`) and refuses
 * item[r] outside [0, items) and len[r] outside [1, T_rows]. */
size_t kk_op_whisper_attn_rows_scratch_bytes(int R, int heads, int T_rows);
int kk_op_whisper_attn_rows(void* stream, int R, int heads, const float* q, const void* kv, int k_off, int v_off, int items, int T_rows, int ld,
                            const int32_t* item, const int32_t* len, float* out, void* scratch, size_t scratch_bytes);
/* The same attention with the keys of a row scattered over the items (a beam's ancestry): owner is a device int32 table [R][T_rows], and key
 * j of row r is read at owner[r][j] * T_rows * ld + j * ld instead of item[r] * T_rows * ld + j * ld.  The arithmetic is that of
 * kk_op_whisper_attn_rows: the output is bit-equal to it on a store that holds the same keys gathered into one item.  Scratch, alignment and
 * refusals as kk_op_whisper_attn_rows; owner[r][j] outside [0, items) for a j < len[r] is refused (the table is read back). */
int kk_op_whisper_attn_rows_owned(void* stream, int R, int heads, const float* q, const void* kv, int k_off, int v_off, int items, int T_rows, int ld,
                                  const int32_t* owner, const int32_t* len, float* out, void* scratch, size_t scratch_bytes);
/* out[m] = act(x[m] W^T + bias) (+ res[m]) for 1 <= M <= 16 rows on the bf16 matrix cores: x fp32 [M][ldx] (rounded to bf16, nearest even), W bf16
 * [N][K] dense (K % 32 == 0, any N), bias fp32 [N] or null, act 0 (none) or 2 (exact GELU), res fp32 [M][ldr] or null.  The result goes to out
 * (fp32 [M][ldo], or null) and / or, rounded to bf16, to row rows_bf16[m] (device int32 [M]; null: row m) of out_bf16 [nrows_bf16][ld_bf16]; a row
 * index outside the store is skipped.  Every weight byte is read once per call. */
int kk_op_whisper_linear_rows(void* stream, int M, int N, int K, const float* x, long long ldx, const void* w, const float* bias, int act,
                              const float* res, long long ldr, float* out, long long ldo, void* out_bf16, long long ld_bf16, const int32_t* rows_bf16,
                              int nrows_bf16);
/* out[r] = table[clamp(tok[r])] + positions[clamp(pos[r])]: table bf16 [n_vocab][D], positions fp32 [n_ctx][D], out fp32 [R][D] */
int kk_op_whisper_embed(void* stream, int R, int D, const int32_t* tok, const int32_t* pos, const void* table_bf16, int n_vocab, const float* positions,
                        int n_ctx, float* out);
/* kk_op_whisper_linear_rows on an MLX affine-quantised W: words uint32 [N][K bits / 32] as the checkpoint holds them (value i of a row
 * in bits [(i % per) bits, ...) of word i / per, per = 32 / bits; 8-byte aligned), pairs float [N][K / group_size][2] = (scale, bias) of every row and
 * group (8-byte aligned); bits 4 or 8, group_size 32, 64 or 128 dividing K.  Each value is decoded in registers to bf16_rne(fp32(q) * scale + bias)
 * (fp32 multiply, fp32 add) and meets the kernel of kk_op_whisper_linear_rows from there on: the result carries the bits that entry gives on the
 * bf16 rounding of the dequantised matrix.  The other arguments and their checks are that entry's. */
int kk_op_whisper_linear_rows_q(void* stream, int M, int N, int K, const float* x, long long ldx, const uint32_t* words, const float* pairs, int group_size,
                                int bits, const float* bias, int act, const float* res, long long ldr, float* out, long long ldo, void* out_bf16,
                                long long ld_bf16, const int32_t* rows_bf16, int nrows_bf16);
/* kk_op_whisper_embed from the quantised table [n_vocab][D] in the layout above (words 4-byte, pairs 8-byte aligned; group_size divides D) */
int kk_op_whisper_embed_q(void* stream, int R, int D, const int32_t* tok, const int32_t* pos, const uint32_t* words, const float* pairs, int group_size,
                          int bits, int n_vocab, const float* positions, int n_ctx, float* out);
/* the token selection of one decode step (decoding.py:302-395 then :260-278 at temperature 0), one launch, no host round trip */
typedef struct kk_whisper_pick_params {
  int32_t n_vocab, eot, blank;           /* blank: the token of " " (220), masked with eot at the first sampled position when suppress_blank */
  int32_t no_timestamps, timestamp_begin;
  int32_t max_initial_timestamp_index;   /* < 0: none */
  int32_t without_timestamps, suppress_blank;
} kk_whisper_pick_params;
typedef struct kk_whisper_pick_state {   /* one per row */
  int32_t last, penultimate;             /* the last two sampled tokens, -1 = none yet */
  int32_t last_timestamp;                /* the last sampled token >= timestamp_begin, -1 = none */
  int32_t ended, count;                  /* eot was sampled; tokens sampled so far */
  float sum_logprob, last_logprob;
  int32_t reserved;
} kk_whisper_pick_state;
/* logits fp32 [B][ldl]; params: ONE device struct; suppress: device bitmask over n_vocab (bit i of word i / 32) or null; state: device [B];
 * tokens: device int32 [B][cap], the chosen token is appended at state.count; next: device int32 [B], the chosen tokens; not_ended: device
 * int32 counter of rows that have not sampled eot (kk_op_whisper_pick_reset sets it to B).  An ended row emits eot and keeps its sum. */
int kk_op_whisper_pick(void* stream, int B, const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                       kk_whisper_pick_state* state, int32_t* tokens, int cap, int32_t* next, int32_t* not_ended);
int kk_op_whisper_pick_reset(void* stream, int B, kk_whisper_pick_state* state, int32_t* not_ended);
/* The same step at temperature > 0 (decoding.py:263-278 behind the same filters): token ~ Categorical(softmax(l / temperature)) over the filtered
 * logits l, logprob = l[token] - logsumexp(l) on the UNTEMPERED l; everything else as kk_op_whisper_pick.  The draw is Gumbel-max in the pass that
 * takes the log-sum-exp: token = argmax_i (l_i / temperature - log(-log u_i)) over the unmasked i, lowest index on ties; u_i = ((r >> 9) + 0.5) 2^-23
 * with r = word i & 3 of Philox4x32-10 on the counter (low state.count, high streams[b], i >> 2, a fixed tag) and the key `seed`.  A row's draws
 * depend on seed, its stream id and its own history alone.  streams: device uint32 [B].  A temperature that is not finite or not > 0 is refused
 * before anything is launched. */
int kk_op_whisper_pick_sampled(void* stream, int B, const float* logits, long long ldl, const kk_whisper_pick_params* params, const uint32_t* suppress,
                               float temperature, uint64_t seed, const uint32_t* streams, kk_whisper_pick_state* state, int32_t* tokens, int cap,
                               int32_t* next, int32_t* not_ended);

typedef struct kk_whisper_text kk_whisper_text;
/* the text fields of ModelDimensions plus the audio side's output shape; n_text_state / n_text_head must be 64, n_text_state a multiple of 128 and
 * at most 2048, n_audio_state == n_text_state */
typedef struct kk_whisper_text_config {
  int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer, n_audio_ctx, n_audio_state;
} kk_whisper_text_config;
int kk_whisper_text_create(const kk_whisper_text_config* cfg, kk_whisper_text** out);
void kk_whisper_text_destroy(kk_whisper_text* m);
/* decoder.* parameters by their MLX checkpoint names, host fp32, Linear weights [out][in]; the keys have no bias */
int kk_whisper_text_load_tensor(kk_whisper_text* m, const char* name, const int64_t* shape, int ndim, const float* data);
/* a matrix of an MLX affine-quantised checkpoint (`{p}.weight` with `{p}.scales` / `{p}.biases`) instead of kk_whisper_text_load_tensor: shape
 * [out][in] of the dequantised matrix, words uint32 [out][in bits / 32], scales / biases fp32 [out][in / group_size]; bits 2, 4 or 8.  What becomes of it
 * is kk_whisper_text_finalize's decision, matrix by matrix. */
int kk_whisper_text_load_quantized(kk_whisper_text* m, const char* name, const int64_t* shape, const uint32_t* words, const float* scales, const float* biases,
                                   int group_size, int bits);
/* rounds every matrix to bf16 (nearest even), one at a time, into ONE device copy (the token embedding serves the gather and the logits); the
 * learned positions, biases and LayerNorm parameters stay fp32.  A quantised matrix stays PACKED -- its words as they are plus one
 * (scale, bias) pair per row and group, decoded inside kk_op_whisper_linear_rows_q / embed_q's kernels -- if its bits are 4 or 8 and its group size is
 * 32, 64 or 128 and divides its input width; any other one, and the two halves of the stacked cross key | value matrix (which set_audio runs on the
 * bf16 conv kernel), are dequantised on the host by the checkpoint's rule, fp32(q) * scale + bias in two roundings, and become bf16 matrices.  Either
 * way the decoder computes the bits it computes on the dequantised checkpoint.  Fails naming a missing or misshapen parameter.  Synchronises `stream`. */
int kk_whisper_text_finalize(kk_whisper_text* m, void* stream);
/* what finalize decided: device bytes of the matrices and of all weights, the count of packed and of bf16 matrices (the stacked cross key | value
 * counts once), and how many quantised tensors were dequantised; kk_whisper_text_weight_fallback(m, i) is "name<TAB>reason" of the i-th of them */
int kk_whisper_text_weight_info(const kk_whisper_text* m, size_t* matrix_bytes, size_t* total_bytes, int* n_packed, int* n_bf16, int* n_fallback);
const char* kk_whisper_text_weight_fallback(const kk_whisper_text* m, int i);
/* the caller's memory: one persistent state buffer per batch (cross and self K/V in bf16, the pick state and token buffers) and a workspace per call */
size_t kk_whisper_text_state_bytes(const kk_whisper_text* m, int B);
size_t kk_whisper_text_workspace_bytes(const kk_whisper_text* m, int B, int S);
/* a new window: audio_features fp32 [B][n_audio_ctx][n_audio_state] rounded to bf16 once, every layer's cross K and V computed once (whisper.py:114-116)
 * into `state`, the rows' position set to 0.  `state` must stay alive and untouched until the next set_audio.  workspace: ..._workspace_bytes(m, B, 1) */
int kk_whisper_text_set_audio(kk_whisper_text* m, void* stream, int B, const float* audio_features, void* state, size_t state_bytes, void* workspace,
                              size_t workspace_bytes);
/* TextDecoder.__call__ on S tokens per row at the rows' position: tokens device int32 [B][S] (null with S = 1: the tokens of the last pick); the self
 * K/V of the new positions are appended, the position advances by S.  logits_out fp32 [B][S][n_vocab] (all_positions) or [B][n_vocab] (the last
 * position only); it must stay alive until the pick that follows.  More than n_text_ctx positions is an error.  Never synchronises. */
int kk_whisper_text_forward(kk_whisper_text* m, void* stream, int B, int S, const int32_t* tokens, float* logits_out, int all_positions, void* workspace,
                            size_t workspace_bytes);
int kk_whisper_text_position(const kk_whisper_text* m);  /* positions consumed since set_audio, -1 before it */
/* back to an earlier position of the same window (0: a new sequence on the cross K/V set_audio made) */
int kk_whisper_text_rewind(kk_whisper_text* m, int position);
/* params (HOST) and the suppress bitmask (HOST, (n_vocab + 31) / 32 words, or null) are copied into the state buffer and the rows' pick state is
 * reset; synchronises.  pick runs kk_op_whisper_pick on the last forward's last-position logits; never synchronises. */
int kk_whisper_text_pick_setup(kk_whisper_text* m, void* stream, const kk_whisper_pick_params* params, const uint32_t* suppress);
int kk_whisper_text_pick(kk_whisper_text* m, void* stream);
/* read back (HOST destinations, synchronise): the count of rows not ended; the token buffers [B][cap] and the rows' states [B] */
int kk_whisper_text_not_ended(kk_whisper_text* m, void* stream, int32_t* out);
int kk_whisper_text_read(kk_whisper_text* m, void* stream, int32_t* tokens, int cap, kk_whisper_pick_state* rows);
/* ---- groups: n_group decoder rows per window on ONE cross K/V slice (best_of) -------------------------------------------------
 * set_audio_groups is set_audio for n_audio windows (audio_features fp32 [n_audio][n_audio_ctx][n_audio_state]) whose cross K/V is projected and
 * kept once per window; the state then carries B = n_audio * n_group rows, row b on window b / n_group, 1 <= n_group <= KK_WHISPER_MAX_GROUP.
 * forward, rewind, pick_setup, pick, not_ended and read work on the B rows; workspace: ..._workspace_bytes(m, B, 1).  set_audio is n_group = 1.
 * The capturing forward refuses a state with n_group > 1. */
#define KK_WHISPER_MAX_GROUP 8
size_t kk_whisper_text_state_bytes_groups(const kk_whisper_text* m, int n_audio, int n_group);
int kk_whisper_text_set_audio_groups(kk_whisper_text* m, void* stream, int n_audio, int n_group, const float* audio_features, void* state,
                                     size_t state_bytes, void* workspace, size_t workspace_bytes);
/* after pick_setup: pick launches kk_op_whisper_pick_sampled with this temperature, seed and the rows' stream ids (HOST uint32 [B], copied;
 * synchronises) until the next pick_setup, which returns the handle to the greedy pick.  Refuses a temperature that is not finite or not > 0. */
int kk_whisper_text_sample_setup(kk_whisper_text* m, void* stream, float temperature, uint64_t seed, const uint32_t* streams);

/* ---- beam search (OpenAI's BeamSearchDecoder on the device) -------------------------------------------------------------------
 * n_audio windows of K = beam_size rows, B = n_audio * K, row b in window b / K.  A step is a forward, kk_op_whisper_beam_topk and
 * kk_op_whisper_beam_select; nothing returns to the host in between.  The self K/V is never moved: owner[b][p] names the physical row that
 * holds position p of beam b, and the step's self-attention reads its keys through it (kk_op_whisper_attn_rows_owned).
 * The device buffers of a beam: */
typedef struct kk_whisper_beam_bufs {
  int32_t n_audio, beam_size;    /* 1 <= beam_size <= KK_WHISPER_MAX_GROUP */
  int32_t max_candidates;        /* finished sequences a window keeps, round(beam_size * patience): 1 .. 2 KK_WHISPER_MAX_GROUP */
  int32_t n_ctx, cap, reserved;  /* positions of an owner row; ids of a token row (tokens [B][cap], fin_tokens rows) */
  int32_t* cand_token;           /* [B][beam_size + 1]: a row's offers in descending log-probability, -1 = none */
  float* cand_logprob;           /* [B][beam_size + 1] */
  int32_t* owner[2];             /* [B][n_ctx] each; select reads owner[flip] and writes owner[flip ^ 1] */
  int32_t* parent;               /* [B]: the row the slot's new prefix extends, -1 for a dead slot */
  float* fin_score;              /* [n_audio][max_candidates]: sum_logprob of a finished sequence */
  int32_t* fin_length;           /* [n_audio][max_candidates]: its tokens before eot */
  int32_t* fin_tokens;           /* [n_audio][max_candidates][cap]: the ids, materialised when it finished */
  int32_t* fin_count;            /* [n_audio] */
  int32_t* complete;             /* [n_audio]: fin_count reached max_candidates */
  int32_t* not_complete;         /* [1]: windows not complete; decremented once per window */
} kk_whisper_beam_bufs;
/* Row b's beam_size + 1 most probable tokens over the logits filtered exactly as kk_op_whisper_pick filters them on state[b]: (token,
 * l[token] - logsumexp(l)) in descending order, equal logits by the lower id, never a masked token; unused slots hold token -1.  The log-sum-exp
 * is the greedy pick's (same order of operations), so the first offer is the greedy pick's token with its log-probability's bits.  A row with
 * every token masked offers (eot, 0) alone; a dead row (state.sum_logprob == -inf) offers nothing.  state is only read. */
int kk_op_whisper_beam_topk(void* stream, int B, int beam_size, const float* logits, long long ldl, const kk_whisper_pick_params* params,
                            const uint32_t* suppress, const kk_whisper_pick_state* state, int32_t* cand_token, float* cand_logprob);
/* bufs: a HOST struct of device pointers.  reset: owner[0][b][p] = b, fin_count = complete = 0, not_complete = n_audio. */
int kk_op_whisper_beam_reset(void* stream, const kk_whisper_beam_bufs* bufs);
/* One BeamSearchDecoder.update per window on the offers in bufs: candidate (row j, rank r) scores state[j].sum_logprob + logprob (fp32); at
 * state.count == 0 only row 0 of a window offers.  The candidates are walked by score descending, then row ascending, then rank ascending: one
 * ending in eot finishes (kept while fin_count < max_candidates, its ids materialised into fin_tokens), any other becomes the next free slot's
 * prefix, until beam_size are saved.  Per slot: parent, next[] and tokens[slot][count] = the token, state = the PARENT's state advanced by the token
 * with sum_logprob = the score, owner[flip ^ 1][slot][p] = owner[flip][parent][p] for p < pos (the positions the parents hold) and the slot itself
 * from pos on.  Slots left over are dead: sum -inf, token eot, own table row.  Token i of a prefix lies at tokens[owner[row][pos - count + i]][i]. */
int kk_op_whisper_beam_select(void* stream, const kk_whisper_beam_bufs* bufs, int flip, int pos, const kk_whisper_pick_params* params,
                              kk_whisper_pick_state* state, int32_t* tokens, int32_t* next);
/* The handle: after set_audio_groups(n_group = beam_size) and pick_setup, beam_setup lays the buffers above out in the caller's beam_state
 * (..._beam_state_bytes; the window state keeps its size) and resets them.  Until the next pick_setup, kk_whisper_text_pick runs top-k and select,
 * and a forward of one position reads the self K/V through the owner table.  not_complete reads the counter of incomplete windows (HOST int32;
 * synchronises).  read (HOST destinations; synchronises): the finished stores -- fin_count [n_audio], fin_score and fin_length [n_audio][max_candidates],
 * fin_tokens [n_audio][max_candidates][cap] -- and the live rows: live_tokens [B][cap] gathered through the table, live_sum and live_length [B]
 * (a dead slot's sum is -inf). */
size_t kk_whisper_text_beam_state_bytes(const kk_whisper_text* m, int n_audio, int beam_size, int max_candidates);
int kk_whisper_text_beam_setup(kk_whisper_text* m, void* stream, int beam_size, int max_candidates, void* beam_state, size_t bytes);
int kk_whisper_text_beam_not_complete(kk_whisper_text* m, void* stream, int32_t* out);
int kk_whisper_text_beam_read(kk_whisper_text* m, void* stream, int cap, int32_t* fin_count, float* fin_score, int32_t* fin_length, int32_t* fin_tokens,
                              int32_t* live_tokens, float* live_sum, int32_t* live_length);

/* ---- row mode: decoder rows that join and leave one running batch -----------------------------------------------------------
 * A second state beside the window of set_audio, on the same weights and the same stream: max_rows <= KK_WHISPER_MAX_ROWS rows, each with its
 * own cross K/V (one window), self K/V, pick parameters, suppress bitmask, pick state, initial-token and sampled-token stores (n_text_ctx ids
 * each) and two kept logits rows.  A row's position is the caller's (initial tokens plus picks).  Opening and using row mode leaves the window
 * state alone.  Every argument error is an error return before anything is launched. */
#define KK_WHISPER_MAX_ROWS 32
typedef struct kk_whisper_rows_item {
  int32_t row, pos, count;  /* decoder row, its first position of this round, tokens of this round */
  int32_t from;             /* >= 0: the tokens are `count` ids at this offset of the row's initial tokens; -1 (count 1): the token of the row's last pick */
  int32_t keep, slot;       /* keep >= 0: the logits of the item's position pos + keep (which out_rows must list) are also copied to the row's kept slot 0 or 1 */
} kk_whisper_rows_item;
/* the caller's memory: one persistent state buffer, and a workspace that serves rounds of up to max_round_rows flat rows in up to max_items items
 * (and admissions); 0 for a bad argument */
size_t kk_whisper_text_rows_state_bytes(const kk_whisper_text* m, int max_rows);
size_t kk_whisper_text_rows_workspace_bytes(const kk_whisper_text* m, int max_round_rows, int max_items);
/* `state` must stay alive and untouched by the caller while row mode is used; every row's ended flag is cleared.  Never synchronises. */
int kk_whisper_text_rows_open(kk_whisper_text* m, void* stream, int max_rows, void* state, size_t state_bytes);
/* a request takes a row: audio_features fp32 [n_audio_ctx][n_audio_state] rounded to bf16 once and every layer's cross K | V computed into THIS
 * row's slice (set_audio's launch with B = 1; the other rows' slices are not touched); tokens (HOST, n ids), params (HOST) and the bitmask (HOST,
 * (n_vocab + 31) / 32 words, or null) are uploaded, the row's pick state is reset.  Synchronises (the host arrays may go away). */
int kk_whisper_text_rows_admit(kk_whisper_text* m, void* stream, int row, const float* audio_features, const int32_t* tokens, int n,
                               const kk_whisper_pick_params* params, const uint32_t* suppress, void* workspace, size_t workspace_bytes);
/* one round of the decoder over R = sum(count) flat rows (item i's rows follow item i - 1's), any mix of prefill and step items; items HOST
 * [n_items], each row at most once; out_rows HOST [n_out]: the distinct flat rows whose logits are wanted, logits_out fp32 [n_out][n_vocab] in
 * that order (it must stay alive until the rows_pick that follows).  The self K/V of the new positions are written.  Refused: a row outside
 * [0, max_rows), never admitted or listed twice; pos + count > n_text_ctx; from + count beyond the row's initial tokens; from = -1 with
 * count != 1 or before the row's pick; a workspace too small for R.  Never synchronises. */
int kk_whisper_text_rows_forward(kk_whisper_text* m, void* stream, const kk_whisper_rows_item* items, int n_items, const int32_t* out_rows, int n_out,
                                 float* logits_out, void* workspace, size_t workspace_bytes);
/* the pick of kk_op_whisper_pick for the listed rows (HOST [n], each once), every row on ITS params, bitmask and state and on the logits of its
 * last position in the last rows_forward (which must have listed it in out_rows); state.ended is the row's flag.  Never synchronises. */
int kk_whisper_text_rows_pick(kk_whisper_text* m, void* stream, const int32_t* rows, int n);
/* the poll: ended HOST int32 [max_rows] (0 for a row that was never admitted); synchronises */
int kk_whisper_text_rows_flags(kk_whisper_text* m, void* stream, int32_t* ended);
/* a row's sampled tokens (HOST [cap]) and pick state (HOST) and, unless null, its two kept logits rows (DEVICE fp32 [2][n_vocab]); synchronises */
int kk_whisper_text_rows_read(kk_whisper_text* m, void* stream, int row, int32_t* tokens, int cap, kk_whisper_pick_state* state, float* kept);
/* initial token `index` of a row from DEVICE memory (the detected language, with no host round trip); never synchronises */
int kk_whisper_text_rows_set_token(kk_whisper_text* m, void* stream, int row, int index, const int32_t* token);
/* after rows_admit (which leaves the row greedy): the row's picks draw at `temperature` on the Philox key `seed` and the stream id `stream_id`, with
 * the bits kk_op_whisper_pick_sampled gives the same logits, parameters, state, seed and stream -- in the same ONE launch of rows_pick that picks
 * the greedy rows.  Refused: temperature <= 0 or not finite, a row outside [0, max_rows) or never admitted.  Synchronises. */
int kk_whisper_text_rows_set_draw(kk_whisper_text* m, void* stream, int row, float temperature, uint64_t seed, uint32_t stream_id);
/* ---- groups of row mode: G rows, 1 <= G <= KK_WHISPER_MAX_GROUP and not necessarily adjacent, that decode ONE window: admitted together,
 * stepped and picked together at one position, released together.  The cross K/V is projected once, into the slices of the leader rows[0]; the other
 * rows read it there.  A group is known by its leader row.  KK_WHISPER_GROUP_PLAIN: every row picks for itself, greedily or (rows_set_draw) on its own
 * draw -- best_of.  KK_WHISPER_GROUP_BEAM (G = beam_size): rows_pick takes the rows' G + 1 best tokens in its one pick launch (the bits of
 * kk_op_whisper_beam_topk) and runs one more launch with a select workgroup per listed beam group (kk_op_whisper_beam_select's walk, slots being the
 * positions in rows[]), each group at its own position and owner-table flip; a beam row's step reads its self keys through its owner row.  The rows'
 * state.ended then carries the group's complete flag, so rows_flags stays the ONE poll.
 * What groups keep (offers, two owner tables and a parent per row; per leader the finished stores of 2 KK_WHISPER_MAX_GROUP sequences of n_text_ctx ids,
 * their count and the complete flag) lives in a second caller-owned buffer, bound after rows_open (every rows_open unbinds it); bind launches nothing.
 * Without it row mode is what it was, and rows_workspace_bytes asked after it includes the round's owner table.
 * Refused, before anything is launched: groups used without the bind call; G outside 1 .. 8; max_candidates of a beam group outside 1 .. 16; a row
 * listed twice or already in a group; rows_admit on a row of a group; a round or a pick that lists some rows of a group and not the others (only the
 * leader may run alone, before the group's first pick: its language detection); rows of a group at different positions; a beam row given initial
 * tokens after its group's first select. */
#define KK_WHISPER_GROUP_PLAIN 0
#define KK_WHISPER_GROUP_BEAM 1
size_t kk_whisper_text_rows_groups_state_bytes(const kk_whisper_text* m, int max_rows);
int kk_whisper_text_rows_groups_bind(kk_whisper_text* m, void* stream, void* state, size_t state_bytes);
/* rows HOST [n_rows]; features, tokens, params and the bitmask as for rows_admit, given to every row; every row's pick state and draw are reset, a beam
 * group's owner rows are identity and its stores empty.  Synchronises once. */
int kk_whisper_text_rows_admit_group(kk_whisper_text* m, void* stream, const int32_t* rows, int n_rows, int kind, const float* audio_features,
                                     const int32_t* tokens, int n, const kk_whisper_pick_params* params, const uint32_t* suppress, int max_candidates,
                                     void* workspace, size_t workspace_bytes);
/* what kk_whisper_text_beam_read returns for one window (HOST destinations; synchronises): fin_count [1], fin_score and fin_length [max_candidates],
 * fin_tokens [max_candidates][cap] (a plain group: fin_count 0, the rest untouched), live_tokens [G][cap] by slot gathered through the owner table,
 * live_sum and live_length [G]; and, unless null, the leader's two kept logits rows (DEVICE fp32 [2][n_vocab]) */
int kk_whisper_text_rows_group_read(kk_whisper_text* m, void* stream, int leader, int cap, int32_t* fin_count, float* fin_score, int32_t* fin_length,
                                    int32_t* fin_tokens, int32_t* live_tokens, float* live_sum, int32_t* live_length, float* kept);
/* the group's rows are free again (each must be admitted anew before it runs); host only */
int kk_whisper_text_rows_group_release(kk_whisper_text* m, int leader);
/* the G + 1 offers of a beam row's last pick (HOST token and logprob [G + 1], descending, unused slots -1 / -inf); synchronises */
int kk_whisper_text_rows_group_offers(kk_whisper_text* m, void* stream, int row, int32_t* token, float* logprob);

/* =====================================================================================================================
 * Whisper, token timestamps from cross-attention: timing.py:19-100, 143-157 and Model.forward_with_cross_qk (csrc/kk_whisper_align.hip,
 * DESIGN 8h).  Device pointers unless stated, work enqueued on `stream`, 0 = OK.  An item's bits depend on that item's inputs alone.
 * ===================================================================================================================== */
/* Raw cross-attention scores (whisper.py:125-130, before the softmax): q fp32 [items * rows][heads * 64], 16-byte aligned; k bf16
 * [items][T_rows][ld] with the keys at channel 0 (the cross store of the text handle, ld = 2 * n_text_state); sel: HOST int32 [n_sel], the
 * heads wanted, any order.  out fp32 [n_sel][items * rows][ldo]: out[j][r][key] = 64^-0.5 q[r][sel[j]] . k[r / rows][key][sel[j]] for
 * key < n_keys <= T_rows; keys at or past n_keys are neither read nor written.  Needs no workspace (the size entry returns 0). */
size_t kk_op_whisper_qk_rows_workspace_bytes(int items, int rows, int n_sel, int n_keys);
int kk_op_whisper_qk_rows(void* stream, int items, int rows, int heads, const float* q, const void* k, int T_rows, int ld, const int32_t* sel, int n_sel,
                          int n_keys, float* out, long long ldo);
/* timing.py:147-155 per item b: softmax over the first n_frames[b] columns of qk * qk_scale for each of n_heads heads and n_rows[b] rows,
 * per (head, column) the mean and population deviation over the rows and (w - mean) / deviation, a median filter of odd width
 * medfilt_width in 1 .. 31 along the columns with reflect padding (skipped when n_frames[b] <= medfilt_width / 2), the mean over the heads
 * summed in head order.  qk fp32 at qk[b * stride_b + h * stride_h + r * ld_in + c]; n_rows, n_frames device int32 [B], each within
 * [1, rows_max] and [1, cols_max] (read back and checked: the entry synchronises).  out fp32 [B][rows_max][ld_out]; cells behind an item's
 * rows and frames are not written.  group: heads per pass (0: the default); the workspace holds one group and the result's bits do not
 * depend on it. */
size_t kk_op_whisper_align_matrix_workspace_bytes(int B, int n_heads, int rows_max, int cols_max, int group);
int kk_op_whisper_align_matrix(void* stream, int B, int n_heads, const float* qk, long long stride_b, long long stride_h, int ld_in, const int32_t* n_rows,
                               int rows_max, const int32_t* n_frames, int cols_max, float qk_scale, int medfilt_width, int group, float* out, int ld_out,
                               void* workspace, size_t workspace_bytes);
/* timing.py:19-44 on its own: out[r][c] = the median of the reflect-padded window of odd `width` in 1 .. 31 around x[r][c], rows of n values
 * (n > width / 2; the reference returns shorter rows unfiltered, so does the Python caller), fp32, row pitches ldx and ldo */
int kk_op_whisper_median_filter(void* stream, long long rows, int n, const float* x, long long ldx, int width, float* out, long long ldo);
/* timing.py:47-95 per item b on x[b] (n_rows[b] x n_cols[b] of fp32 [B][..][ld] at item stride stride_b; negate: on -x): fp32 costs, the
 * reference's tie rule, its backtrace.  text_indices, time_indices int32 [B][rows_max + cols_max]: the path in forward order, length[b]
 * entries; first_cols int32 [B][rows_max]: per row the column of the path's first entry there (time_indices[jumps]).  n_rows, n_cols device
 * int32 [B] within [1, rows_max] and [1, cols_max] (read back and checked: the entry synchronises); cols_max at most 15360. */
size_t kk_op_whisper_dtw_workspace_bytes(int B, int rows_max, int cols_max);
int kk_op_whisper_dtw(void* stream, int B, const float* x, long long stride_b, int ld, const int32_t* n_rows, int rows_max, const int32_t* n_cols, int cols_max,
                      int negate, int32_t* text_indices, int32_t* time_indices, int32_t* length, int32_t* first_cols, void* workspace, size_t workspace_bytes);
/* kk_whisper_text_forward with all_positions = 1 that also captures: pairs HOST int32 [n_pairs][2] of (layer, head); after each listed
 * layer's cross_attn.query Linear the raw scores of its listed heads go to qk_out fp32 [B][n_pairs][S][n_keys], pair p in slot p.  The
 * logits are the bits of the plain forward.  qk_bytes: at least what the size entry returns.  workspace: as for the plain forward. */
size_t kk_whisper_text_qk_bytes(const kk_whisper_text* m, int B, int S, int n_pairs, int n_keys);
int kk_whisper_text_forward_qk(kk_whisper_text* m, void* stream, int B, int S, const int32_t* tokens, float* logits_out, const int32_t* pairs, int n_pairs,
                               int n_keys, float* qk_out, size_t qk_bytes, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* KOKORO_HIP_H */

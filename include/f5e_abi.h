/* f5e_abi.h -- C ABI of libf5e_hip.so: the MI355X (gfx950) kernels of the F5E-TTS flow-matching inference hot path.
 *
 * The reference (kaleo996/F5E-TTS) has no FFI for this path: it is a chain of PyTorch nn.Module calls.  Each entry
 * point below therefore replaces a *PyTorch op sequence*; the comment on each names the reference lines
 * (paths relative to src/f5_tts/).  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions (lower side)
 *   - plain pointers and ints only; every pointer is a DEVICE pointer unless the name says "host".
 *   - the caller owns every buffer (workspace included); the library never allocates, frees or synchronises inside
 *     an op, so every op is capturable into a hipGraph (f5e_graph_*).
 *   - hipStream_t is passed as void* (the value of torch.cuda.current_stream().cuda_stream).
 *   - row-major; "ld*" = leading dimension in ELEMENTS; bf16 = 16-bit brain float, f32 = IEEE binary32.
 *   - return value: 0 = F5E_OK, negative = error; message via f5e_last_error() (thread local).  No C++ exception
 *     crosses the ABI.  Re-entrant: no global mutable state besides the thread-local error string.
 */
#ifndef F5E_ABI_H_
#define F5E_ABI_H_

#ifdef __cplusplus
extern "C" {
#endif

#define F5E_ABI_VERSION 2   /* 2: f5e_ln_fuse.row_stats / f5e_ln_finalize / F5E_WS_LN_ROWSTATS removed, f5e_sample_loop added */

/* The library is built with -fvisibility=hidden: exactly the functions declared here are exported. */
#if defined(__GNUC__)
#define F5E_API __attribute__((visibility("default")))
#else
#define F5E_API
#endif

enum { F5E_OK = 0, F5E_ERR_BAD_SHAPE = -1, F5E_ERR_UNSUPPORTED = -2, F5E_ERR_HIP = -3 };

/* activation selectors */
enum { F5E_ACT_NONE = 0, F5E_ACT_SILU = 1, F5E_ACT_GELU_ERF = 2, F5E_ACT_GELU_TANH = 3, F5E_ACT_RELU = 4, F5E_ACT_MISH = 5 };
/* the element type of a 16-bit weight operand (the _w16 entry points) */
enum { F5E_W_FP16 = 1, F5E_W_BF16 = 2 };

#ifdef F5E_STREAM_T
typedef F5E_STREAM_T f5e_stream; /* library build: the real hipStream_t (same ABI: one pointer) */
#else
typedef void* f5e_stream; /* hipStream_t */
#endif

F5E_API int f5e_abi_version(void);
F5E_API const char* f5e_last_error(void);
/* 0 when the current HIP device is gfx950; F5E_ERR_UNSUPPORTED otherwise (host call, no kernel launch). */
F5E_API int f5e_check_device(void);

/* ---------------------------------------------------------------- bf16 MFMA GEMMs (hot loop) ----------------- */

/* out[M][N] = act(A[M][K] . W[N][K]^T + bias).  A, W bf16; bias f32[N] or NULL; out bf16 (out_f32 = 0) or f32.
 * act: F5E_ACT_NONE or F5E_ACT_GELU_TANH.  K % 64 == 0, N % 4 == 0; lda, ldw multiples of 8, ldo a multiple of 4 and, with
 * M > 1, at least N (the same holds for ldr and f5e_ln_fuse.ld_xs below); nothing is written outside [0, M) x [0, N).
 * tile_hint: 0 = auto, or force a tile family: 1 = 128x128, 2 = 128x64, 3 = 64x64, 9 = the 256x256 ping-pong kernel (what
 * auto picks from 44 row tiles of 256 on).
 * Replaces: FeedForward project_in + GELU(tanh) (model/modules.py:348-349,625), proj_out (backbones/dit.py:470). */
F5E_API int f5e_gemm_bf16_bias(f5e_stream st, const void* A, int lda, const void* W, int ldw, const float* bias, void* out,
                       int ldo, int M, int N, int K, int act, int out_f32, int tile_hint);

/* resid[m][n] += gate[(m / rows_per_seq) % gate_rows][n] * (A . W^T + bias)[m][n], skipped for rows whose position
 * (m % rows_per_seq) >= seq_len[m / rows_per_seq] when seq_len != NULL.  gate is read at
 * gate + (*eval_ptr) * eval_stride when eval_ptr != NULL.
 * Replaces: attn.to_out + masked_fill + "x + gate_msa * attn" (modules.py:494-501,635) and
 *           ff.ff[2] + "x + gate_mlp * ff" (modules.py:350,639). */
F5E_API int f5e_gemm_bf16_gate_residual(f5e_stream st, const void* A, int lda, const void* W, int ldw, const float* bias,
                                float* resid, int ldr, const float* gate, int gate_stride, int gate_rows,
                                const int* eval_ptr, int eval_stride, int rows_per_seq, const int* seq_len, int M,
                                int N, int K, int tile_hint);

/* Fused to_q/to_k/to_v (+bias) + rotary embedding on the first rope_heads heads of q and k.  W = [3*heads*64][K]
 * (rows: q | k | v).  Outputs: q, k [S][heads][n_pad][64] bf16, vt [S][heads][64][n_pad] bf16 (V transposed).
 * cos_sin: [rows_per_seq][32][2] f32 from f5e_rope_table.  Pad rows/columns of q/k/vt are never written: the
 * caller zero-fills them once.
 * q is stored PRE-SCALED by log2(e) / sqrt(64) (folded in after RoPE, before the bf16 rounding): f5e_flash_attn's scores
 * are then in the log2 domain with no multiply per element (csrc/attention.hip).
 * q_norm_w / k_norm_w: optional f32[64] RMSNorm weights applied per head before RoPE (qk_norm = "rms_norm", eps 1e-6).
 * Replaces: modules.py:452-461 (projections + head split), :464-467 (qk norm) and :470-480 (apply_rotary_pos_emb). */
F5E_API int f5e_gemm_bf16_qkv_rope(f5e_stream st, const void* A, int lda, const void* W, int ldw, const float* bias, void* q,
                           void* k, void* vt, int n_pad, int heads, int rope_heads, const float* cos_sin,
                           const float* q_norm_w, const float* k_norm_w, int rows_per_seq, int M, int K,
                           int tile_hint);

/* Fused AdaLayerNorm for small row counts (batch-1 sampling): the LayerNorm + modulate launch in front of a linear
 * (modules.py:308-314 + :452-454; :637 + :349; :329-335 + dit.py:470) is folded into the GEMMs either side of it.
 *   producer = the gate+residual GEMM before it: next to x_new it writes xs = bf16((x_new - o) (1 + next_scale[n])) and,
 *     per row and 64-column tile, (mean - o, M2) of x_new into stats_out [M][N / 64][2], o = row_mean[m];
 *   consumer = the linear after it, run on A = xs:  out = rstd (acc - mean' c[n]) + d[n]  with the per-evaluation
 *     tables c[n] = sum_k W[n][k] (1 + scale[k]),  d[n] = sum_k W[n][k] shift[k] + bias[n]  (row r =
 *     (m / rows_per_seq) % cd_rows, advanced by (*eval_ptr) * cd_eval_stride), mean' (relative to o) / rstd combined from
 *     the `parts` tile statistics (Chan's formula, fixed order); pass bias = NULL to the GEMM.  Its column tile 0 then moves
 *     row_mean[m] += mean', so the next producer centres with the row's current mean.
 *   Why centred: bf16(x (1 + scale)) would round at the size of the row's OFFSET, and the error of the normalised result
 *     would grow like |mean| / std (off-centre rows of trained networks).  Row means drift slowly from norm to norm, so
 *     with o = the mean as of the previous norm the rounding is at the size of the row's spread, as in the unfused form.
 * Only one side is used per launch; leave the other side's pointers NULL.  Runs on the 64x64 tile family whatever M (the
 * fusion pays at small row counts, where the LayerNorm launches are pure latency; at large M keep f5e_layernorm).
 * Consumer limits: parts a multiple of 4 up to 16 (D <= 1024), cd_rows == 1 (one table row per evaluation). */
typedef struct f5e_ln_fuse {
  const float* stats; int parts;                       /* consumer */
  const float* c; const float* d; int cd_stride; int cd_rows; int cd_eval_stride;
  const int* eval_ptr; int rows_per_seq; float eps;
  void* xs_out; int ld_xs; const float* next_scale;    /* producer (next_scale uses the gate's strides / rows) */
  float* stats_out;
  float* row_mean;                                     /* both sides: [M] f32 centring offsets, see below */
} f5e_ln_fuse;

F5E_API int f5e_gemm_bf16_bias_ln(f5e_stream st, const void* A, int lda, const void* W, int ldw, const float* bias, void* out,
                          int ldo, int M, int N, int K, int act, int out_f32, int tile_hint, const f5e_ln_fuse* ln);
F5E_API int f5e_gemm_bf16_gate_residual_ln(f5e_stream st, const void* A, int lda, const void* W, int ldw, const float* bias,
                                   float* resid, int ldr, const float* gate, int gate_stride, int gate_rows,
                                   const int* eval_ptr, int eval_stride, int rows_per_seq, const int* seq_len, int M,
                                   int N, int K, int tile_hint, const f5e_ln_fuse* ln);
F5E_API int f5e_gemm_bf16_qkv_rope_ln(f5e_stream st, const void* A, int lda, const void* W, int ldw, const float* bias,
                              void* q, void* k, void* vt, int n_pad, int heads, int rope_heads, const float* cos_sin,
                              const float* q_norm_w, const float* k_norm_w, int rows_per_seq, int M, int K,
                              int tile_hint, const f5e_ln_fuse* ln);

/* ---------------------------------------------------------------- attention ---------------------------------- */

/* o[S*rows_per_seq][ldo] (bf16, column = head*64 + d) = softmax(q k^T / 8 + keymask) v, keys >= kv_len[s] masked.
 * kv_len[s] above rows_per_seq counts as rows_per_seq; kv_len[s] = 0 (no key at all) gives all-zero rows for sequence s.
 * q as f5e_gemm_bf16_qkv_rope writes it: already multiplied by log2(e) / 8, so the kernel computes 2^(q' k^T - max).
 * q, k, v use the fragment-major layouts documented in csrc/attention.hip; splits: KV splits per 32-query tile
 * (0 = auto, 1, 2 or 4; -1 = the LDS-shared 128-query kernel that auto picks for large problems).
 * Replaces: F.scaled_dot_product_attention + transpose/reshape (modules.py:482-492). */
F5E_API int f5e_flash_attn(f5e_stream st, const void* q, const void* k, const void* vt, void* o, int ldo, const int* kv_len,
                   int S, int H, int rows_per_seq, int n_pad, int splits);

/* MMDiT joint attention: per (sequence s, head h) the keys / values are the audio keys 0 .. kv_len[s]-1 followed by the
 * text keys 0 .. Nt-1 (kv_len NULL = all N audio keys; text keys are never masked), and
 *   o_x[s*N  + i][h*64 + d] (ldo_x) = softmax(qx k^T / 8) v   for the audio queries i < N,
 *   o_c[s*Nt + j][h*64 + d] (ldo_c) = softmax(qc k^T / 8) v   for the text queries j < Nt  (o_c NULL: skipped, qc unused).
 * qx / kx / vx and qc / kc / vc are two sets of f5e_gemm_bf16_qkv_rope outputs (fragment-major, q pre-scaled by log2(e) / 8):
 * audio [S][H][n_pad_x][64] written with rows_per_seq = N, text [S][H][n_pad_c][64] written with rows_per_seq = Nt and
 * its own RoPE table from position 0.  splits: KV splits per 32-query tile (0 = auto, 1, 2 or 4).
 * Replaces: the concatenation of the two streams, the padded key mask and F.scaled_dot_product_attention + the split of
 * its output (modules.py:688-710). */
F5E_API int f5e_joint_attn(f5e_stream st, const void* qx, const void* kx, const void* vx, const void* qc, const void* kc,
                   const void* vc, void* o_x, int ldo_x, void* o_c, int ldo_c, const int* kv_len, int S, int H, int N,
                   int n_pad_x, int Nt, int n_pad_c, int splits);

/* ---------------------------------------------------------------- normalisation ------------------------------ */

/* y = LN(x; eps)  [* gamma + beta]  [* (1 + scale[r]) + shift[r]],  r = (row / rows_per_seq) % mod_rows.
 * x f32 [rows][D]; y bf16 or f32.  D % 256 == 0, D <= 2048.  scale/shift advance by (*eval_ptr) * eval_stride.
 * Replaces: AdaLayerNorm / ff_norm modulation / AdaLayerNorm_Final (modules.py:308-314,329-335,637) and the affine
 * LayerNorms of ConvNeXtV2Block (modules.py:253,264) and Vocos. */
F5E_API int f5e_layernorm(f5e_stream st, const float* x, int ldx, void* y, int ldy, int y_bf16, const float* gamma,
                  const float* beta, const float* scale, const float* shift, int mod_stride, int mod_rows,
                  int rows_per_seq, const int* eval_ptr, int eval_stride, int rows, int D, float eps);

/* First producer of the fused-AdaLN chain (block 0 has no GEMM in front of its norm): row_mean[row] = the row's exact
 * mean, xs = bf16((x - mean) (1 + scale[r])) and stats [rows][parts][2] holding `parts` equal shares (0, M2 / parts) of
 * each row's statistics (tile means relative to row_mean). */
F5E_API int f5e_adaln_pre(f5e_stream st, const float* x, int ldx, void* xs, int ld_xs, const float* scale, int mod_stride,
                  int mod_rows, int rows_per_seq, const int* eval_ptr, int eval_stride, float* stats, int parts,
                  float* row_mean, int rows, int D);

/* x_transformers.RMSNorm used by UNetT (backbones/unett.py:151,161,178): y = x / max(||x||_2, 1e-12) * sqrt(D) * g. */
F5E_API int f5e_l2norm(f5e_stream st, const float* x, int ldx, void* y, int ldy, int y_bf16, const float* g, int rows, int D);

/* GRN over the sequence axis (modules.py:225-234): x, y f32 [B][T][C]; gx_ws f32 [B][C] scratch. */
F5E_API int f5e_grn(f5e_stream st, const float* x, float* y, float* gx_ws, const float* gamma, const float* beta, int B, int T,
            int C);

/* ---------------------------------------------------------------- exact-fp32 GEMM (once per call) ------------ */

/* C[m][n] = ((act(sum_k actA(A[m % a_rows][k]) W[n][k] + bias[n])) * ch_scale[n] + addend[m % add_rows][n]) * row_scale[m]
 * written to out (f32) and/or out_bf16.  K, lda, ldw multiples of 4.  NULL skips a term.  Rows of A and W may overlap
 * (lda, ldw >= 0); with M > 1, ldo and ldo_bf16 must be at least N, and ld_add too when add_rows > 1.  Any alignment of the
 * pointers and the other leading dimensions is taken (16-byte friendly operands take the faster paths).
 * Replaces the fp32 F.linear calls of TimestepEmbedding, AdaLN emb, TextEmbedding, PPGEmbedding, InputEmbedding.proj
 * (x columns per step; cond/text/ppg columns once per call) and Vocos. */
F5E_API int f5e_gemm_f32(f5e_stream st, const float* A, int lda, int a_rows, int a_act, const float* W, int ldw,
                 const float* bias, int act, const float* ch_scale, const float* addend, int ld_add, int add_rows,
                 const float* row_scale, float* out, int ldo, void* out_bf16, int ldo_bf16, int M, int N, int K);

/* ---------------------------------------------------------------- convolutions ------------------------------- */

/* One grouped Conv1d(D, D, 31, groups, padding = 15) + Mish of ConvPositionEmbedding (modules.py:167-190, called with
 * mask=None at backbones/dit.py:176).  x bf16 [S*N][ldx]; w_packed bf16 [groups][31][64 oc][64 ic], zero padded when
 * D/groups (16, 32, 48 or 64) is below 64.  mode 0: out_bf16 = mish(conv + bias); mode 1: out_f32 = mish(..) + resid.
 * Refused before any launch: D % groups != 0 or D/groups outside {16, 32, 48, 64}; ldx not a multiple of 8; ldo, ldo32 or
 * ldr not a multiple of 4; with more than one row (S * N > 1) any of ldx and the mode's ldo / ldo32, ldr below D; x,
 * w_packed, bias, out_f32 or resid not 16-byte aligned, out_bf16 not 8-byte aligned; a mode without its output (mode 1:
 * and its residual).  Only columns [0, D) of the S * N rows of x / resid are read and of the output written; bias holds D
 * floats. */
F5E_API int f5e_convpos(f5e_stream st, const void* x, int ldx, const void* w_packed, const float* bias, int mode,
                void* out_bf16, int ldo, float* out_f32, int ldo32, const float* resid, int ldr, int S, int N, int D,
                int groups);

/* Depthwise Conv1d(C, C, 7, padding 3, groups C), channels-last f32 [B][T][C]; w_t = weight transposed to [7][C]. */
F5E_API int f5e_dwconv7(f5e_stream st, const float* x, const float* w_t, const float* bias, float* y, int B, int T, int C);

/* col[b][t][j*Cin + ic] = x[b][t + j - pad][ic] (0 outside [0, T)). */
F5E_API int f5e_im2col(f5e_stream st, const float* x, float* col, int B, int T, int Cin, int ksize, int pad);

/* Strided Conv2d(C, C, [kt, kf], stride) without padding, channels-last, as an implicit GEMM on the exact-fp32 MFMA
 * (csrc/subsample.hip): the second / third convolution of the wenet Conv2dSubsampling4 / 6 / 8 stacks.
 *   y[b][to][fo][n] = act(bias[n] + sum_{i, j, c} x[b][to * stride + i][fo * stride + j][c] * w[n][i][j][c])
 * x f32 [B][T_in][F_in][C], w f32 [C][kt][kf][C] (the torch weight [C_out][C_in][kt][kf] permuted on the host), bias f32 [C]
 * or NULL, y f32 [B][T_out][F_out][C] with T_out = (T_in - kt) / stride + 1, F_out = (F_in - kf) / stride + 1.  act:
 * F5E_ACT_NONE or F5E_ACT_RELU.  C % 16 == 0, kt, kf in 1..8, all pointers 16-byte aligned, B * T_in * F_in < 2^31.  No
 * workspace: the loader gathers the K = kt * kf * C operand row from x (kt contiguous runs of kf * C floats). */
F5E_API int f5e_conv2d_sub_f32(f5e_stream st, const float* x, const float* w, const float* bias, float* y, int B, int T_in,
                       int F_in, int C, int kt, int kf, int stride, int act);

/* ---------------------------------------------------------------- sampler elementwise ------------------------ */

/* out[e] = cat(sin(a), cos(a)), a = (scale * t[e]) * freqs[k]   (modules.py:154-161; freqs = host constant [dim/2]).
 * t f32 [E], out f32 [E][dim], dim even and >= 4; a is one fp32 product of a product (no add: nothing to contract) and
 * goes through sincosf, as n * inv_freq[i] does in f5e_rope_table (inv_freq f32 [half], out f32 [N][half][2]). */
F5E_API int f5e_sinus_embed(f5e_stream st, const float* t, const float* freqs, float* out, int E, int dim, float scale);
/* out[n][i] = (cos, sin)(n * inv_freq[i])   (x_transformers RotaryEmbedding.forward_from_seq_len) */
F5E_API int f5e_rope_table(f5e_stream st, const float* inv_freq, float* out, int N, int half);
/* out[b][n] = (table[ids[b][n]] + pos[min(n, max_pos-1)]) * keep[b][n]   (backbones/dit.py:68-80).  table f32
 * [table_rows][TD]; an id outside [0, table_rows) is clamped (nn.Embedding raises IndexError there: the host side checks
 * ids that start on the host, the clamp only keeps device-resident garbage from reading outside the table). */
F5E_API int f5e_text_gather(f5e_stream st, const int* ids, const float* table, const float* pos, const float* keep, float* out,
                    int B, int N, int TD, int max_pos, int table_rows);
/* v = p0 | p0 + (p0 - p1) w0 | w0 (p2 - p1) + w1 (p1 - p0) + p0   (mode 0 | 1 | 2; p_k = pred + k * branch_stride);
 * dst = base + coef[*eval_ptr] * v; traj (optional) gets a copy.   (model/cfm.py:447, :187, :310 + Euler/midpoint)
 * done_ctr (optional, one zero-initialised u32): the last workgroup to finish does ++*eval_ptr and re-zeroes it. */
F5E_API int f5e_ode_update(f5e_stream st, const float* pred, long long branch_stride, int mode, float w0, float w1,
                   const float* base, float* dst, float* traj, const float* coef, int* eval_ptr, unsigned* done_ctr,
                   long long n);
/* Same, with the trajectory row picked on the device: traj row (*eval_ptr + 1) / traj_div of [rows][traj_stride] floats
 * (euler: traj_div 1; midpoint's second stage: 2), so a captured step needs no per-step copy.  traj_stride 0 = plain. */
F5E_API int f5e_ode_update_traj(f5e_stream st, const float* pred, long long branch_stride, int mode, float w0, float w1,
                        const float* base, float* dst, float* traj, long long traj_stride, int traj_div,
                        const float* coef, int* eval_ptr, unsigned* done_ctr, long long n);
F5E_API int f5e_advance_eval(f5e_stream st, int* eval_ptr);
/* out = mask ? cond : y   (cfm.py:476); mask u8 [rows], tensors f32 [rows][C] */
F5E_API int f5e_stitch(f5e_stream st, const float* cond, const float* y, const unsigned char* mask, float* out, long long rows,
               int C);
F5E_API int f5e_cast_bf16(f5e_stream st, const float* x, void* y, long long n);
/* y f32 = x bf16 (exact).  Used to rebuild the fused-AdaLN tables from the bf16 weights the MFMA kernels read. */
F5E_API int f5e_cast_f32(f5e_stream st, const void* x, float* y, long long n);
/* out = a x + b y + c  (y may be NULL).  (1 - t_inter) y0 + t_inter cond of duplicate_test (model/cfm.py:460-465). */
F5E_API int f5e_axpby(f5e_stream st, const float* x, const float* y, float* out, float a, float b, float c, long long n);
/* GumbelVectorQuantizer eval forward (model/modules.py:881-950): logits f32 [rows][ld] (groups * num_vars used) ->
 * targets i32 [rows][groups] (first maximal index), out f32 [rows][groups * var_dim] gathered from vars f32
 * [(combine_groups ? 1 : groups) * num_vars][var_dim]; stats (optional) f32[2] = (code_perplexity, prob_perplexity). */
F5E_API int f5e_vq_eval(f5e_stream st, const float* logits, int ld, const float* vars, int combine_groups, float* out,
                int* targets, float* stats, int rows, int groups, int num_vars, int var_dim);

/* Monotonic alignment search (durpred/monotonic_align/core.py maximum_path_jit, called through DiT.align_text_ppg,
 * model/backbones/dit.py:309-331): the best monotonic path through logp f32 [B][Ty][ld] (row = frame y, column = token x;
 * sequence b at logp + b * batch_stride, elements), for the device lengths t_y[b] frames and t_x[b] tokens.
 *   Q[0][0] = L[0][0];  Q[y][x] = L[y][x] + max(x < y ? Q[y-1][x] : -1e9, x > 0 ? Q[y-1][x-1] : -1e9)   (fp32, one add per
 *   cell) over the band max(0, t_x - (t_y - y)) <= x <= min(t_x - 1, y); backtrack from (t_y - 1, t_x - 1): frame y takes
 *   token i, then i -= 1 iff i > 0 and (i == y or Q[y-1][i] < Q[y-1][i-1]) -- a tie stays on the token.
 * token_of_frame i32 [B][Ty]: the token of every frame, -1 for y >= t_y[b]; durations (optional) i32 [B][Tx]: frames per
 * token, 0 for x >= t_x[b].  A sequence without a monotonic path (t_x < 1, t_y < t_x, or a length beyond Ty / Tx) gets
 * all -1 / all 0.  logp is not modified (the reference accumulates in place).  workspace: f5e_mas_workspace_bytes(B, Ty, Tx)
 * bytes of caller-owned scratch, 8-byte aligned, contents irrelevant.  Tx <= 4096.  No allocation, no synchronisation. */
F5E_API int f5e_mas_workspace_bytes(int B, int Ty, int Tx, unsigned long long* bytes_out_host);
F5E_API int f5e_mas_path(f5e_stream st, const float* logp, long long batch_stride, int ld, const int* t_y, const int* t_x,
                 int* token_of_frame, int* durations, void* workspace, unsigned long long workspace_bytes, int B, int Ty,
                 int Tx);

/* Polyphase windowed-sinc sample-rate conversion (torchaudio.transforms.Resample, sinc_interp_hann, as restated by
 * infer/audio.py::resample; reference infer/utils_infer.py:445-447, ppg/ppg_model.py:156-158) for the reduced ratio
 * orig : new:   y[b][f * new + p] = sum_{k < taps} bank[p][k] * x[b][f * orig + k - width],   taps = 2 * width + orig,
 * x read as 0 outside [0, n).  x f32 [B][ld_x] (n used), bank f32 [new][taps] (the caller's filter bank, computed once per
 * ratio), y f32 [B][ld_y] (n_out = ceil(new * n / orig) written per row; the gap ld_y - n_out is not touched).  fp32 FMA,
 * eight interleaved partial sums per output.  F5E_ERR_BAD_SHAPE for orig, new, n < 1, n_out != ceil(new * n / orig) or
 * ld < length; F5E_ERR_UNSUPPORTED beyond 4096 taps.  No allocation, no synchronisation. */
F5E_API int f5e_resample(f5e_stream st, const float* x, long long ld_x, const float* bank, int orig, int new_, int width,
                 float* y, long long ld_y, int B, int n, int n_out);

/* CTC forced alignment (csrc/ctc.hip; reference ppg/wenet/utils/ctc_util.py::forced_align, batched, on the device).
 * scores f32 [B][T][V]: log-probabilities OR raw logits of the CTC head (per-frame constants cancel), batch stride
 * `batch_stride`, row stride `ld` >= V, unit class stride, only read.  labels i32 [B][ld_labels] (L used).  t_len / l_len:
 * DEVICE int [B].  Viterbi over the blank-interleaved sequence (S = 2 l + 1 states; stay, s-1, and s-2 where the label
 * differs from the one before it), fp32, one max and one add per cell, the first maximum winning; the path ends in the last
 * blank unless the last label scores strictly higher.  State 0 can only stay (the reference's negative index there wraps to
 * the last state).  align i32 [B][T]: the class of every frame's state (blank or a label), -1 for t >= t_len.
 * Optional tok_start / tok_end i32 [B][L]: first / one-past-last frame of every label's own state (0 / 0 for a label the
 * path never visits, which needs -inf in the scores); score f32 [B]: alpha of
 * the chosen end state.  A sequence without a path (l_len < 1, t_len < l_len + adjacent equal labels, a label outside
 * [0, V), lengths beyond T / L) gets -1 / 0 / -inf rows; the other sequences are untouched.  workspace:
 * f5e_ctc_align_workspace_bytes(B, T, L) bytes of caller-owned scratch, 8-byte aligned, contents irrelevant.
 * T <= 16384, L <= 2047.  No allocation, no synchronisation. */
F5E_API int f5e_ctc_align_workspace_bytes(int B, int T, int L, unsigned long long* bytes_out_host);
F5E_API int f5e_ctc_align(f5e_stream st, const float* scores, long long batch_stride, int ld, const int* labels, int ld_labels,
                  const int* t_len, const int* l_len, int blank, int* align, int* tok_start, int* tok_end, float* score,
                  void* workspace, unsigned long long workspace_bytes, int B, int T, int L, int V);

/* CTC best-path decoding (reference ppg/asr_model.py:450-458): per frame the argmax over V of scores (layout as above; the
 * lowest index among equal maxima), per sequence the collapse "keep frame t iff its id is not blank and differs from frame
 * t-1's", compacted into hyp i32 [B][T] (padded with -1) and hyp_len i32 [B].  Frames t >= t_len[b] (DEVICE int [B]) take the
 * id pad_id when pad_id >= 0 (the reference fills them with eos BEFORE collapsing) and are skipped when pad_id = -1.
 * Optional frame_logp f32 [B][T]: max - logsumexp of EVERY row of the buffer (padded frames included, as the reference's
 * topk_prob).  T <= 16384.  No allocation, no synchronisation. */
F5E_API int f5e_ctc_greedy(f5e_stream st, const float* scores, long long batch_stride, int ld, const int* t_len, int blank,
                   int pad_id, int* hyp, int* hyp_len, float* frame_logp, int B, int T, int V);

/* CTC likelihood of a transcript (csrc/ctc.hip; reference ppg/wenet/transformer/ctc.py::CTC.forward, i.e.
 * torch.nn.CTCLoss, per utterance and negated).  scores / labels / t_len / l_len: the layout and meaning of f5e_ctc_align
 * (lengths are DEVICE int [B]; scores is only read), raw logits OR log-probabilities: every frame is normalised here
 * (x - logsumexp of its row), so both give the same value up to rounding.  logp f32 [B] = log of the sum over ALL CTC paths
 * of labels[b][:l_len] through frames [0, t_len) = -CTCLoss(reduction "none"): the forward recurrence over the
 * blank-interleaved sequence (S = 2 l + 1 states; stay, s-1, and s-2 where the label differs from the one before it) in
 * fp32 with logaddexp = max + log1p(exp(-|d|)); true -inf log-probabilities are legal and never give NaN.  Adjacent equal
 * labels are ordinary input (they need t_len >= l_len + repeats); l_len = 0 is legal (the all-blank path, the sum of the
 * blank log-probabilities; L = 0 with labels NULL too).  A sequence without a path (t_len < l_len + repeats, a label outside
 * [0, V), l_len < 0 or > L, t_len < 1 or > T) gets -inf, where torch returns +inf loss; the other sequences are untouched.
 * workspace: f5e_ctc_loss_workspace_bytes(B, T) bytes (f32 [B][T], the normaliser of every frame, written by a first launch
 * of one wave per frame) of caller-owned scratch, 4-byte aligned, contents irrelevant.  T <= 16384, L <= 2047, B <= 65535.
 * No gradient.  No allocation, no synchronisation. */
F5E_API int f5e_ctc_loss_workspace_bytes(int B, int T, unsigned long long* bytes_out_host);
F5E_API int f5e_ctc_loss(f5e_stream st, const float* scores, long long batch_stride, int ld, const int* labels, int ld_labels,
                 const int* t_len, const int* l_len, int blank, float* logp, void* workspace,
                 unsigned long long workspace_bytes, int B, int T, int L, int V);

/* CTC prefix beam search (csrc/ctc_beam.hip; reference ppg/asr_model.py:461-546, batched, on the device).  scores f32
 * [B][T][V] in the layout of f5e_ctc_align, raw logits OR log-probabilities: every frame is normalised here as
 * (x - max) - log1p(sum over the other classes of exp(x - max)), so both give the same lists and scores.  t_len: DEVICE
 * int [B].  Per frame t < t_len: the first prune keeps the `beam` best classes of the frame; for every kept class s with
 * log-probability ps and every beam prefix (pb, pnb):
 *   s = blank:               prefix      pb  <- logaddexp(pb + ps, pnb + ps);
 *   s = the prefix's last:   prefix      pnb <- pnb + ps,   and   prefix + (s)   pnb <- pb + ps;
 *   otherwise:               prefix + (s)   pnb <- logaddexp(pb + ps, pnb + ps),
 * contributions to one prefix being combined with logaddexp (fp32, log1p(exp(-|d|)) form); a prefix nothing contributed to
 * is dropped.  The second prune keeps the `beam` best prefixes by logaddexp(pb, pnb).  The start is the empty prefix with
 * (0, -inf).  Ties: among equal scores of a frame the lower class index comes first; among equal prefix totals the
 * candidates are ordered "beam entries that keep their prefix, in beam order (best first), then the new prefixes by (rank of
 * the parent entry, rank of the class in the frame's first prune)" -- a fixed order of this kernel; the reference's is its
 * dict's insertion order.
 * hyp i32 [B][beam][ld_hyp]: the prefixes, best first, padded with -1; a prefix longer than ld_hyp leaves its first ld_hyp
 * tokens.  hyp_len i32 [B][beam]: the true lengths.  score f32 [B][beam] = logaddexp(pb, pnb).  t_len = 0 gives the empty
 * prefix (length 0, score 0) in row 0; rows the search did not fill (those, and every row of a sequence with t_len outside
 * [0, T]) are -1 / length -1 / -inf; the other sequences are untouched.  workspace: f5e_ctc_beam_workspace_bytes(B, T, beam)
 * bytes (16 per sequence, frame and beam slot) of caller-owned scratch, 8-byte aligned, contents irrelevant.
 * 1 <= beam <= 16, beam <= V, T <= 16384, B <= 65535.  No allocation, no synchronisation. */
F5E_API int f5e_ctc_beam_workspace_bytes(int B, int T, int beam, unsigned long long* bytes_out_host);
F5E_API int f5e_ctc_beam(f5e_stream st, const float* scores, long long batch_stride, int ld, const int* t_len, int blank,
                 int beam, int* hyp, int ld_hyp, int* hyp_len, float* score, void* workspace,
                 unsigned long long workspace_bytes, int B, int T, int V);

/* The same search, resumable (csrc/ctc_beam.hip): the frames of a sequence arrive in chunks, and after the last chunk hyp /
 * hyp_len / score equal those of ONE f5e_ctc_beam call on all the frames bit for bit, however the frames were cut (empty
 * chunks included): a frame's first prune depends on that frame alone, the recurrence is the same code doing the same fp32
 * operations in the same order, and trie node numbers use the absolute frame index.
 * state: opaque, caller-owned DEVICE memory of f5e_ctc_beam_state_bytes(B, T_cap, chunk_cap, beam) bytes, 8-byte aligned; per
 * sequence the frames consumed, the beam (node, parent, last token, length, hash, pb, pnb, entry count), the trie of T_cap x
 * beam nodes and the first-prune scratch of one chunk (chunk_cap x beam pairs); sizes and offsets are 64-bit.
 * f5e_ctc_beam_state_init: one small launch (no host-side memset, capturable) that puts every sequence at the empty prefix
 * and records the geometry; the rest of the state needs no initial value.
 * f5e_ctc_beam_chunk: scores f32 [B][T_chunk][V] with the strides of f5e_ctc_beam; n_frames DEVICE int [B] = how many of the
 * chunk's frames belong to each sequence (0: idle this call).  Two launches: the first prune of the chunk, then one workgroup
 * per sequence that loads its beam, runs n_frames[b] frames, stores the beam and adds to the frames consumed.  hyp / hyp_len
 * / score: all null (no readout), or all given: the result so far in the layout of f5e_ctc_beam (hyp i32 [B][beam][ld_hyp]);
 * the readout does not change the state, so it can be repeated (a call with n_frames = 0 is a pure readout).
 * B, T_cap, chunk_cap and beam are those of state_init (the host needs them for the grid and the offsets); T_chunk <=
 * chunk_cap.  A sequence FAILS when n_frames[b] < 0, n_frames[b] > T_chunk or consumed + n_frames[b] > T_cap: it gets -1 /
 * length -1 / -inf rows in this call and in every later one (the state marks it dead until the next state_init), writes
 * nothing outside its own share of the state, and the other sequences are untouched.  A state whose recorded geometry is not
 * the call's (or that was never initialised) fails every sequence and is not written.  1 <= beam <= 16, beam <= V,
 * chunk_cap <= 16384, T_cap <= 2^20, B <= 65535.  No allocation, no synchronisation. */
F5E_API int f5e_ctc_beam_state_bytes(int B, int T_cap, int chunk_cap, int beam, unsigned long long* bytes_out_host);
F5E_API int f5e_ctc_beam_state_init(f5e_stream st, void* state, unsigned long long state_bytes, int B, int T_cap,
                            int chunk_cap, int beam);
F5E_API int f5e_ctc_beam_chunk(f5e_stream st, const float* scores, long long batch_stride, int ld, const int* n_frames,
                       int T_chunk, int V, int blank, int beam, void* state, unsigned long long state_bytes, int* hyp,
                       int ld_hyp, int* hyp_len, float* score, int B, int T_cap, int chunk_cap);

/* out[r] = logits[r][target[r]] - logsumexp(logits[r][0..V)) for `rows` rows of row stride ld (fp32, max-subtracted), one wave
 * per row: the terms of the reference's rescoring sum (ppg/asr_model.py:660-670) without the copy of [N, U, V]
 * log-probabilities to the host.  target[r] < 0 gives 0 (a padded position), target[r] >= V gives NaN.  No allocation, no
 * synchronisation. */
F5E_API int f5e_token_logp(f5e_stream st, const float* logits, long long ld, const int* target, float* out, long long rows,
                   int V);
/* out[r][v] = x[r][v] - logsumexp(x[r][0..V)) (torch.log_softmax over the last axis; fp32, max-subtracted), one wave per row;
 * row strides ldx, ldo >= V; out may be x.  No allocation, no synchronisation. */
F5E_API int f5e_log_softmax_rows(f5e_stream st, const float* x, long long ldx, float* out, long long ldo, long long rows,
                         int V);

/* ---------------------------------------------------------------- mel / vocoder ------------------------------ */

/* out[B][T][n_mels] = log(clamp(|STFT(wav)| . fb, 1e-5)), T = 1 + nw / hop, reflect-padded, centred (modules.py:75-101).
 * window f32 [1024]; twiddle f32 [512][2] = (cos, -sin)(2 pi k / 1024); fb f32 [513][n_mels].  wav f32 [B][ldw], nw
 * samples of each row read.  Refused: n_fft != 1024, nw <= 512 (the reflection), n_mels > 256, ldw < nw with B > 1.  out is
 * written in full and must hold B * T * n_mels floats: the caller sizes it by T = 1 + nw / hop.  A clamped output is the
 * correctly rounded log(1e-5f) = 0xC13834F1 (a stored constant, not the device's logf of 1e-5). */
F5E_API int f5e_stft_logmel(f5e_stream st, const float* wav, int nw, int ldw, const float* window, const float* twiddle,
                    const float* fb, float* out, int B, int n_fft, int hop, int n_mels);
/* The same, bit for bit, with the filterbank handed over banded: filter m is non-zero on FFT bins [lo, lo + cnt) only
 * (fb_band i32 [n_mels][3] = lo, cnt, offset into fb_compact; fb_compact f32 [nnz <= 2048] = those weights, filter after
 * filter).  What MelSpec uses; the dense form above stays for arbitrary filterbanks. */
F5E_API int f5e_stft_logmel_banded(f5e_stream st, const float* wav, int nw, int ldw, const float* window, const float* twiddle,
                           const float* fb_compact, const int* fb_band, int nnz, float* out, int B, int n_fft, int hop,
                           int n_mels);
/* The banded form generalised for the BigVGAN front-end (reference model/modules.py:30-72): frame f covers samples
 * [f hop - pad_left, f hop - pad_left + 1024) of wav, reflect-padded (no edge repeat; pad_left < nw), T frames
 * (caller-chosen), magnitude sqrt(re^2 + im^2 + mag_eps).  pad_left = 512, T = 1 + nw / hop, mag_eps = 0 is
 * f5e_stft_logmel_banded; BigVGAN uses pad_left = (1024 - hop) / 2, T = nw / hop, mag_eps = 1e-9. */
F5E_API int f5e_stft_logmel_banded_ex(f5e_stream st, const float* wav, int nw, int ldw, const float* window,
                              const float* twiddle, const float* fb_compact, const int* fb_band, int nnz, float* out, int B,
                              int n_fft, int hop, int n_mels, int pad_left, int T, float mag_eps);
/* Vocos ISTFTHead tail: z f32 [B*T][ldz] (513 log-magnitudes | 513 phases) -> out f32 [B][hop * (T - 1)];
 * frames_ws f32 [B*T][1024] scratch (written in full).  Refused: n_fft != 1024, T < 2, ldz < 1026, a hop that does not
 * divide 1024, and hop > 512: at hop = 1024 the Hann envelope under out[b][512 + 1024 f] is zero (0 / 0; torch.istft
 * refuses the same case as a NOLA violation). */
F5E_API int f5e_istft_head(f5e_stream st, const float* z, int ldz, const float* window, const float* twiddle, float* frames_ws,
                   float* out, int B, int T, int n_fft, int hop);

/* ---------------------------------------------------------------- BigVGAN-v2 generator (vocoder_bigvgan.py) --- */

/* Activation1d (anti-aliased SnakeBeta, channels-last): x f32 [B][L][C] -> y [B][L][C], bf16 (out_f32 = 0) or f32.
 * 2x upsample (replicate-pad 5, 2 * conv_transpose1d stride 2 with f_up[12], crop 15 / 15), s = u + inv_beta[c] *
 * sin^2(alpha[c] u), 2x downsample (replicate-pad 5 / 6, stride-2 conv1d with f_dn[12]).  alpha / inv_beta f32 [C] are
 * the final per-channel factors (exp() of a log-scale parameter and 1 / (beta + 1e-9) applied by the caller). */
F5E_API int f5e_bigvgan_act(f5e_stream st, const float* x, void* y, int out_f32, const float* alpha, const float* inv_beta,
                    const float* f_up, const float* f_dn, int B, int L, int C);
/* Conv1d(Cin -> N, ksz taps, dilation dil, zero padding pad, output length L) on bf16 operands, fp32 accumulation:
 * x bf16 [B][L][Cin] (Cin % 4 == 0), w_packed bf16 [roundup(N, 64)][ksz][Cin_pad] (Cin_pad % 32 == 0, zero-padded),
 * bias f32 [N] (optional).  v = acc + bias + resid (resid f32 [B][L][N], optional); out f32 [B][L][N] = v (optional);
 * sum f32 [B][L][N] = (sum_init ? 0 : sum) + sum_scale * v (optional).  ksz <= 11, (ksz - 1) dil <= 64. */
F5E_API int f5e_bigvgan_conv(f5e_stream st, const void* x, const void* w_packed, const float* bias, const float* resid,
                     float* out, float* sum, float sum_scale, int sum_init, int B, int L, int Cin, int Cin_pad, int N,
                     int ksz, int dil, int pad);
/* conv_post: out f32 [B][L] = clamp(conv1d(a, w) + bias, -1, 1) (or tanh), a f32 [B][L][C], w f32 [ksz][C] (odd ksz,
 * pad (ksz - 1) / 2), bias f32 [1] optional. */
F5E_API int f5e_bigvgan_post(f5e_stream st, const float* a, const float* w, const float* bias, float* out, int B, int L, int C,
                     int ksz, int use_tanh);

/* ---------------------------------------------------------------- PPG extractor front ------------ */

/* torchaudio.compliance.kaldi.fbank as the reference calls it (ppg/wenet/dataset/feats.py:66-72): frame f = samples
 * [f shift, f shift + win) of wav * in_scale (snip_edges), minus its mean, pre-emphasised (x[j] - preemph x[j-1], x[-1] = x[0]),
 * times window[win] (povey), zero-padded to 512, |rfft|^2 . fb[257][n_mels], log(max(., eps)).
 * out f32 [B][T][n_mels], T = 1 + (nw - win) / shift.  twiddle f32 [256][2] = (cos, -sin)(2 pi k / 512). */
F5E_API int f5e_kaldi_fbank(f5e_stream st, const float* wav, int nw, int ldw, const float* window, const float* twiddle,
                    const float* fb, float* out, int B, int win, int shift, int n_mels, float in_scale, float preemph,
                    float eps);
/* y[r][c] = x[r][c] * sigmoid(x[r][C + c])   (F.glu over channels, ppg/wenet/transformer/convolution.py:119) */
F5E_API int f5e_glu(f5e_stream st, const float* x, int ldx, float* y, int ldy, long long rows, int C);
/* Depthwise Conv1d(C, C, K, padding (K-1)/2, groups C), channels-last f32 [B][T][C]; w_t = weight transposed to [K][C];
 * keep (optional f32 [B][T], 0/1): frames with keep == 0 count as zeros (convolution.py:100-101).  Odd K <= 31. */
F5E_API int f5e_dwconv(f5e_stream st, const float* x, const float* w_t, const float* bias, const float* keep, float* y, int B,
               int T, int C, int K);
/* y[r][k] = softmax_k(scale * x[r][k], k < len) for k < len, 0 for len <= k < ldy; len = kv_len[r / rows_per_seq] or L
 * (ppg/wenet/transformer/attention.py:75-87). */
F5E_API int f5e_softmax_rows(f5e_stream st, const float* x, int ldx, float* y, int ldy, const int* kv_len, long long rows,
                     int rows_per_seq, int L, float scale);
/* The depthwise convolutions of a chunk-trained (streaming) conformer (convolution.py:81-134); layouts as f5e_dwconv, y must
 * not alias x.  causal == 0: taps t + j - (K-1)/2 that lie in t's chunk [c*chunk, (c+1)*chunk) and in [0, T) (chunk <= 0:
 * the whole sequence), odd K <= 31.  causal != 0: taps t-(K-1) .. t, any K <= 31; positions before the sequence read
 * fill[c] (optional f32 [C], GLU(pointwise_conv1.bias); null: 0); chunk is ignored. */
F5E_API int f5e_dwconv_stream(f5e_stream st, const float* x, const float* w_t, const float* bias, const float* fill, float* y,
                      int B, int T, int C, int K, int causal, int chunk);
/* Fused relative-position attention (attention.py:172-222, no rel_shift), exact fp32, one launch for all sequences, heads
 * and 16-query tiles:  out[b*T + t][h*dk + d] = sum_k softmax_k(scale * (qu[.][h*dk + :] . k[b*T + k][h*dk + :] +
 * qu[.][H*dk + h*dk + :] . pos[k][h*dk + :])) * v[b*T + k][h*dk + d]  over the keys k of the query's band.
 *   qu  [B*T][>= 2*H*dk]  (q + pos_bias_u | q + pos_bias_v);  k, v, out [B*T][>= H*dk];  pos [>= T][>= H*dk] (row = key index)
 *   kv_len (optional int32 [B]): keys >= kv_len[b] are not attended; query rows >= kv_len[b] produce zeros
 *   chunk > 0: a query in chunk c = t / chunk attends keys [max(0, (c - left_chunks) * chunk), min((c + 1) * chunk, len))
 *              (wenet/utils/mask.py subsequent_chunk_mask); chunk <= 0: full context; left_chunks < 0: all left chunks.
 *              Key tiles outside a query tile's band are skipped, so the work is linear in T for a bounded band.
 *   q_begin:   only query rows t >= q_begin of each sequence are computed and written (a chunk appended to cached rows)
 * Head dims dk = 16, 32, 64, 128; row strides multiples of 4 floats, qu / k / pos / out 16-byte aligned.  No allocation,
 * no synchronisation. */
F5E_API int f5e_relpos_attn(f5e_stream st, const float* qu, int ldq, const float* k, int ldk, const float* pos, int ldp,
                    const float* v, int ldv, float* out, int ldo, const int* kv_len, int B, int T, int H, int dk,
                    int q_begin, int chunk, int left_chunks, float scale);
/* Plain masked attention with separate query and key counts (attention.py:79-111: the attention decoder's self- and source
 * attention), exact fp32, one launch for all sequences, heads and 16-query tiles (the wave tile of f5e_relpos_attn):
 *   out[b*Tq + i][h*dk + d] = sum_j softmax_j(scale * q[b*Tq + i][h*dk + :] . k[b*Tk + j][h*dk + :]) * v[b*Tk + j][h*dk + d]
 * over the visible keys j of query i:  j < kv_len[b] (optional DEVICE int32 [B], clamped to [0, Tk]; null: Tk), and j <= i
 * when causal != 0 (which needs Tq == Tk).  EVERY query row i < Tq is computed -- kv_len limits keys, not queries -- and a
 * query with no visible key yields zeros (the reference's masked_fill(mask, 0.0) after its softmax).
 *   q, out [B*Tq][>= H*dk];  k, v [B*Tk][>= H*dk];  each operand has its own row stride.
 * Head dims dk = 16, 32, 64, 128; row strides of q, k and out multiples of 4 floats, q / k / out 16-byte aligned.  No
 * allocation, no synchronisation. */
F5E_API int f5e_mha_f32(f5e_stream st, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* out,
                int ldo, const int* kv_len, int B, int Tq, int Tk, int H, int dk, int causal, float scale);

/* ---- attention-decoder beam search (reference ASRModel.recognize, ppg/asr_model.py:309-414), one decode step at a time.
 *
 * Cached single-query self-attention of decode step p (0-based position of the token being fed) for R = B * beam rows:
 *   kc, vc  f32 [R][Umax][>= H*dk], caller-owned per decoder layer: element (r, j, c) at r*row_stride + j*pos_stride + c
 *   qkv     f32 [R][ld_qkv >= 3*H*dk]: the step's fused projection q | k | v of every row
 *   anc     i32 [R][ld_anc >= p] or NULL: anc[r][j] = the row in which row r's hypothesis stood when position j was fed
 * For row r and head h the kernel FIRST files k and v of the step in slot [r][p] of the caches, then leaves
 *   out[r][h*dk + d] = sum_{j=0..p} softmax_j(scale * q . k_j) * v_j[d]
 * where position j < p is read from cache row anc[r][j] (clamped to [0, R); row r itself when anc is NULL) and position p
 * from the row's own qkv.  Every position 0..p is visible (the reference's subsequent mask has no padding term).
 * Writes: out rows, and slot [r][p] of kc / vc by row r alone -- no other cache byte is touched, and no launch reads a slot
 * it writes, so there is no race inside a launch; a search that calls this once per step and layer writes every slot once.
 * Passing the table for every layer follows the beam's ancestry (a cache-free recompute gives the same numbers); passing
 * NULL leaves each cache with its row index, which is what the reference's un-reordered per-layer cache computes for its
 * layers >= 1.  Neither moves a cache row.
 * Limits: 0 <= p < Umax <= 4096; head dims dk = 16, 32, 64, 128; R, H <= 65535; ld_qkv, row_stride and pos_stride multiples
 * of 4 floats, qkv and kc 16-byte aligned.  fp32 throughout.  No allocation, no synchronisation. */
F5E_API int f5e_attn_decode_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                        int pos_stride, const int* anc, int ld_anc, float* out, int ldo, int R, int Umax, int H, int dk, int p,
                        float scale);
/* One step of the beam search (asr_model.py:374-403) for B utterances of `beam` rows each, one workgroup per utterance.
 *   logits  f32 [B*beam][ld_logits >= V]: RAW decoder outputs of step p; the kernel normalises each row itself (fp32,
 *           max-subtracted: (x - max) - log(sum exp(x - max)), as f5e_log_softmax_rows)
 *   score   f32 [B*beam], in and out: the rows' accumulated log-probabilities.  Start: 0, -inf, ..., -inf per utterance
 *   hyp_in / anc_in  i32 [B*beam][ld]: the tables before the step (hyp column 0 = sos; hyp columns 0..p, anc columns < p)
 *   hyp_out / anc_out i32 [B*beam][ld]: the tables after it; DIFFERENT buffers (the gather crosses rows)
 *   last    i32 [B*beam] out: the class every new row ends in (hyp_out column p + 1, contiguous for the next embedding)
 *   alive   i32 [B] out: rows of the utterance not ending in eos after this step
 *   done_at i32 [B] in/out, -1 at the start: set to p ONCE, at the first step after which alive[b] is 0
 * Semantics: a row is finished iff p > 0 and its last token hyp_in[r][p] is eos (sos may equal eos: step 0 has no finished
 * row).  First prune: the `beam` largest classes of every unfinished row; a finished row contributes the single candidate
 * (score + 0, eos) and beam - 1 candidates at -inf.  Candidate value = score + log p in fp32.  Second prune: the `beam`
 * largest of the utterance's beam^2 candidates become rows 0..beam-1 in descending order; new row q gets its parent's
 * hypothesis with the class appended at column p + 1 and its parent's ancestry with the parent's (global) row at column p.
 * Ties: lower class first in the first prune, lower (parent row, rank) first in the second.
 * Containment: columns > p + 1 of hyp_out, columns > p of anc_out and every input table are untouched.
 * Limits: 1 <= beam <= 16, beam <= V, 0 <= eos < V, ld >= p + 2, B <= 65535.  No allocation, no synchronisation. */
F5E_API int f5e_beam_step(f5e_stream st, const float* logits, long long ld_logits, float* score, const int* hyp_in,
                  const int* anc_in, int* hyp_out, int* anc_out, int ld, int* last, int* alive, int* done_at, int B, int V,
                  int beam, int p, int eos);

/* ---------------------------------------------------------------- fused DiT evaluation ----------------------- */

typedef struct f5e_dit_block_weights {
  const void* w_qkv;  const float* b_qkv;  /* bf16 [3*H*64][D], f32 [3*H*64] */
  const void* w_out;  const float* b_out;  /* bf16 [D][H*64] */
  const void* w_ff1;  const float* b_ff1;  /* bf16 [FF][D] */
  const void* w_ff2;  const float* b_ff2;  /* bf16 [D][FF] */
  const float* q_norm_w; const float* k_norm_w; /* f32 [64] each, or NULL (qk_norm off) */
} f5e_dit_block_weights;

typedef struct f5e_dit_plan {
  int S, B, N, n_pad, D, H, rope_heads, FF, L, mel;
  int mod_rows;               /* rows of the modulation table per evaluation (1, or B for per-item times) */
  /* inputs */
  const float* y;             /* [B*N][mel] f32: network input (ODE state) */
  const float* w_x; int ldw_x;/* input_embed.proj.weight[:, :mel] f32 */
  const float* in_const;      /* [S*N][D] f32: cond/text/ppg part of the input projection + bias, per branch */
  const void* convpos_w1; const float* convpos_b1;
  const void* convpos_w2; const float* convpos_b2;
  int convpos_groups;         /* ConvPositionEmbedding groups (16 in the reference) */
  const float* rope_cs;       /* [N][32][2] */
  const int* seq_len;         /* [S] valid frames per sequence, or NULL (= N, the reference's mask=None case) */
  const float* mod;           /* [E][mod_rows][L*6*D + 2*D] f32 */
  const int* eval_ptr;        /* device int: current evaluation index into mod */
  const f5e_dit_block_weights* blocks; /* HOST array [L] */
  const void* w_proj; const float* b_proj; /* bf16 [mel][D], f32 [mel] */
  const float* w_skip;        /* long_skip_connection.weight f32 [D][2D] or NULL (backbones/dit.py:264,466-467) */
  float* skip_res; float* skip_tmp; /* [S*N][D] f32 each, only with w_skip */
  /* workspace (caller-owned, sizes in elements) */
  float* h0; void* h0_bf16; void* c1;   /* [S*N][D] f32 / bf16 / bf16 */
  float* x;                              /* [S*N][D] f32 residual stream */
  void* hn;                              /* [S*N][D] bf16 */
  void* q; void* k; void* vt;            /* [S][H][n_pad][64] x2, [S][H][64][n_pad] bf16, zero-filled once */
  void* ao;                              /* [S*N][H*64] bf16 */
  void* ff;                              /* [S*N][FF] bf16 */
  float* pred;                           /* [S*N][mel] f32 */
  /* optional instrumentation (eager launches only, never inside graph capture) */
  void* timer;                           /* from f5e_timer_create, or NULL */
  int timer_op;                          /* F5E_OP_* op class to bracket with HIP events; a NEGATIVE value -(mask) selects
                                            every class whose bit (1 << F5E_OP_x) is set in mask */
  /* fused AdaLN (f5e_ln_fuse): 2 L + 1 LayerNorm launches become one f5e_adaln_pre.  Needs no long skip / qk_norm. */
  int fuse_ln;                           /* 0 = separate LayerNorm launches */
  float* ln_stats;                       /* [S*N][D / 64][2] f32 workspace */
  float* ln_rowmean;                     /* [S*N] f32 workspace: the rows' centring offsets (f5e_ln_fuse.row_mean) */
  const float* cd;                       /* [E][mod_rows][cd_stride] f32: per block c_qkv | d_qkv | c_ff1 | d_ff1 */
  int cd_stride;                         /*   (3 H 64, 3 H 64, FF, FF), then c_proj | d_proj (mel, mel)          */
  /* batch-1 chains (fused AdaLN path): a few grid-tail workgroups of each block launch pull the weights of the launch after
   * next into the 256 MB Infinity Cache (the 646 MB of block weights cycle through it, so every GEMM otherwise streams
   * from HBM).  Pure performance hint: results never depend on it. */
  int mall_prefetch;
} f5e_dit_plan;

/* Workspace planner (SURVEY 8b lower side): byte size and 256-byte-aligned offset of every caller-owned buffer of
 * f5e_dit_plan inside ONE arena of `total` bytes.  Only the shape fields of `shape` are read (S, N, D, H, FF, mel, fuse_ln
 * and whether w_skip is set); n_pad = N rounded up to 64 is what the plan must carry.  Buffers that the shape does not
 * need (ln_stats without fuse_ln, skip_* without w_skip) get size 0.  q, k and vt must be zero-filled once by the caller
 * (their pad rows are never written).  Host call, no kernel launch, no allocation. */
enum { F5E_WS_H0 = 0, F5E_WS_H0_BF16, F5E_WS_C1, F5E_WS_X, F5E_WS_HN, F5E_WS_Q, F5E_WS_K, F5E_WS_VT, F5E_WS_AO, F5E_WS_FF,
       F5E_WS_PRED, F5E_WS_LN_STATS, F5E_WS_SKIP_RES, F5E_WS_SKIP_TMP, F5E_WS_LN_ROWMEAN, F5E_WS_COUNT };
typedef struct f5e_dit_workspace {
  int n_pad;
  unsigned long long bytes[F5E_WS_COUNT];
  unsigned long long offset[F5E_WS_COUNT];
  unsigned long long total;
} f5e_dit_workspace;
F5E_API int f5e_workspace_bytes(const f5e_dit_plan* shape, f5e_dit_workspace* out_host);

enum { F5E_OP_NONE = 0, F5E_OP_INPROJ = 1, F5E_OP_CONVPOS = 2, F5E_OP_LN = 3, F5E_OP_QKV = 4, F5E_OP_ATTN = 5,
       F5E_OP_OUT = 6, F5E_OP_FF1 = 7, F5E_OP_FF2 = 8, F5E_OP_FINAL = 9 };

/* HIP-event timer: host-side helpers (these DO allocate / synchronise; they are not ops).  f5e_dit_forward records
 * one start/stop pair around every launch of plan->timer_op, on the stream the kernels are launched on. */
F5E_API int f5e_timer_create(int capacity, void** timer_out);
F5E_API int f5e_timer_destroy(void* timer);
F5E_API int f5e_timer_reset(void* timer);
F5E_API int f5e_timer_read(void* timer, float* ms_out_host, int max_out, int* count_out_host);
F5E_API int f5e_timer_read_ops(void* timer, int* ops_out_host, int max_out, int* count_out_host); /* op class of each pair */

#ifdef F5E_TOOLS
/* Diagnostics, TOOLS build only (make -C f5e-tts_amd/csrc tools-lib -> libf5e_hip_tools.so; tools/convpos_time.py): while
 * buf != NULL, f5e_convpos launches a build of its kernels that writes 8 timestamps per workgroup.  This is
 * process-wide mutable state, which is why the shipped libf5e_hip.so neither contains nor exports it. */
F5E_API void f5e_debug_convpos_trace(void* buf);
/* The same for the 4-way split launches of f5e_flash_attn (tools/attn_timeline.py): 8 timestamps per workgroup and wave. */
F5E_API void f5e_debug_attn_trace(void* buf);
#endif

/* One DiT.sample evaluation for S = branches * B sequences (backbones/dit.py:452-470 after the cached embeddings). */
F5E_API int f5e_dit_forward(f5e_stream st, const f5e_dit_plan* plan);

/* The fixed-grid ODE loop of the samplers (model/cfm.py:430-471 with torchdiffeq's euler / midpoint): enqueues
 * `steps` steps of   [f5e_dit_forward(eval_a); f5e_ode_update]   (euler) or
 *                    [f5e_dit_forward(eval_a); update y_mid = y + coef . v; f5e_dit_forward(eval_b); update y = y + coef . v]
 * (midpoint; eval_b reads y_mid) on `st`.  Nothing is synchronised or allocated: wrap the call in f5e_graph_begin / _end to
 * get the whole loop as ONE executable graph (what the Python host does), or call it with steps = 1 per step.
 * Per-step scalars come from device tables indexed by *eval_ptr (the plans' modulation / fused-AdaLN tables, `coef`), which
 * every update advances by itself through done_ctr -- so one enqueued step serves the whole grid. */
typedef struct f5e_loop_plan {
  const f5e_dit_plan* eval_a;  /* the step's (first) evaluation: y = the ODE state, pred = all branches' outputs */
  const f5e_dit_plan* eval_b;  /* midpoint: second evaluation (y = y_mid); NULL = euler */
  int steps;                   /* steps to enqueue */
  int mode; float w0, w1;      /* guidance combine of f5e_ode_update: 0 plain, 1 CFG, 2 three-branch */
  long long n;                 /* elements of the ODE state: B * N * mel */
  float* y;                    /* [n] state: y(t_k) in, y(t_k + steps) out */
  float* y_mid;                /* [n] midpoint scratch (eval_b->y), NULL for euler */
  const float* pred;           /* [branches][n]: where the evaluations leave their outputs, branch 0 first */
  const float* coef;           /* [E] step coefficients per evaluation: dt (euler) | dt / 2, dt (midpoint) */
  int* eval_ptr;               /* device int: evaluation counter (also eval_a / eval_b ->eval_ptr) */
  unsigned* done_ctr;          /* device u32, zero: arrival counter of the self-advancing update */
  float* traj;                 /* optional [rows][n]: row (evaluation + 1) / evals_per_step receives y after every step */
} f5e_loop_plan;
F5E_API int f5e_sample_loop(f5e_stream st, const f5e_loop_plan* loop);

/* ---------------------------------------------------------------- ECAPA-TDNN speaker encoder (csrc/ecapa.hip) */
/* The head of the reference's SIM metric (eval/ecapa_tdnn.py, eval/utils_eval.py::run_sim) from the stack of WavLM hidden
 * states to the embedding.  Channels-last f32 [B][T][C]; len = DEVICE int [B] or NULL (every row has T frames), clamped to
 * [0, T].  Frames t >= len[b] are written as ZERO by every op below and are left out of every statistic, so row b of a padded
 * batch equals the B = 1 run on its first len[b] frames whatever the padding holds (finite or not: it is never read by
 * f5e_layer_mix_inorm, and every later tensor is zero there).  The 1x1 / k5 convolutions and the linears are f5e_gemm_f32
 * (+ f5e_im2col) with BatchNorm(eval) folded into ch_scale / addend and `mask` as row_scale.  No allocation, no
 * synchronisation, nothing read back: all of it is capturable. */

/* x[b][t][f] = InstanceNorm_t(sum_l softmax(feature_weight)_l * hs[l][b][t][f] + 1e-6)   (ecapa_tdnn.py:284-295): biased
 * variance about the mean over t < len[b], eps 1e-5, no affine.  hs f32 [L][B][T][F] is read ONCE (first launch: mix,
 * written to x); the statistics come from the mixed values (second launch, in place on x).  mask f32 [B][T] = t < len[b].
 * L <= 256, F % 4 == 0, hs and x 16-byte aligned. */
F5E_API int f5e_layer_mix_inorm(f5e_stream st, const float* hs, const float* feature_weight, const int* len, float* x,
                        float* mask, int L, int B, int T, int F);

/* Steps [first, first + count) of Res2Conv1dReluBn (ecapa_tdnn.py:37-53; scale 8, so C = 8 w): for i = 0..6
 * sp = x_i (i = 0) or sp + x_i;  sp = bn_i(relu(conv_i(sp)));  y_i = sp;  and y_7 = x_7 (written when first + count = 7),
 * x_i / y_i = columns [i w, (i + 1) w).  conv_i: w -> w, 3 taps at `dilation`, zero padded; frames outside [0, len[b]) are
 * zero at EVERY step.  w_packed f32 [7][w][3 w] with k = tap * w + ic; bias / bn_scale / bn_shift f32 [7][w].  One launch:
 * a workgroup owns 16 output frames and recomputes a halo of count * dilation frames per side, so T is unbounded; the step
 * weights and two [16 + 2 count dilation][w] images live in LDS, which bounds w (160 KiB: w = 64 takes 89 KiB at
 * dilation 4; w = 128 does not fit).  first > 0 reads y_{first-1} of an EARLIER launch (seven launches of one step each
 * give the same bits).  x and y must not alias.  C % 8 == 0. */
F5E_API int f5e_res2_dconv(f5e_stream st, const float* x, int ldx, float* y, int ldy, const float* w_packed, const float* bias,
                   const float* bn_scale, const float* bn_shift, const int* len, int B, int T, int C, int dilation,
                   int first, int count);

/* mean[b][c] = mean over t < len[b] of x[b][t][c]  (SE_Connect, ecapa_tdnn.py:81); std_out (NULL to skip) =
 * sqrt(unbiased variance + 1e-10) (the global context of AttentiveStatsPool, :148-149; len < 2 gives 1e-5, where torch
 * gives NaN).  mean / std_out rows have stride ld_out.  C, ldx, ld_out multiples of 4, 16-byte aligned. */
F5E_API int f5e_time_stats(f5e_stream st, const float* x, int ldx, const int* len, float* mean, float* std_out, int ld_out,
                   int B, int T, int C);

/* out[b][t][c] = x[b][t][c] * sigmoid(gate[b][c]) + resid[b][t][c]   (ecapa_tdnn.py:83-84, :127); gate f32 [B][C] holds
 * the LOGITS of SE_Connect.linear2.  C and every ld a multiple of 4, 16-byte aligned. */
F5E_API int f5e_se_scale(f5e_stream st, const float* x, int ldx, const float* gate, const float* resid, int ldr, float* out,
                 int ldo, int B, int T, int C);

/* x[b][t][j] = tanh(x[b][t][j] + add[add_rows == 1 ? 0 : b][j]) in place   (ecapa_tdnn.py:155: the bias of pooling.linear1,
 * plus, with global_context_att, the row's constant context term).  add_rows = 1 or B. */
F5E_API int f5e_bias_tanh(f5e_stream st, float* x, int ldx, const float* add, int ld_add, int add_rows, int B, int T, int N);

/* Attentive statistics pooling (ecapa_tdnn.py:157-161): alpha = softmax over t < len[b] of logits[b][t][c];
 * out[b] = [sum alpha x | sqrt(clamp(sum alpha x^2 - mean^2, min = 1e-9))], f32 [B][2 C].  One pass with an online softmax
 * (running maximum, rescaled sums), so logits of any finite size neither overflow nor lose the row; the second moment is
 * carried about the running weighted mean (the same quantity without the cancellation of the two sums).  len = 0 gives
 * [0 | sqrt(1e-9)].  C, ldx, ldl multiples of 4, 16-byte aligned. */
F5E_API int f5e_attn_stats_pool(f5e_stream st, const float* x, int ldx, const float* logits, int ldl, const int* len,
                        float* out, int B, int T, int C);

/* ---------------------------------------------------------------- WavLM upstream (csrc/wavlm.hip, csrc/ppg_attention.hip) */
/* The upstream of the SIM metric (WavLM-large through s3prl in the reference, eval/ecapa_tdnn.py:171-199): from 16 kHz audio
 * to the stack of hidden states that f5e_layer_mix_inorm takes.  fp32, channels-last, eval mode.  The strided convolutions 1-6
 * of the extractor, the projections and the feed-forward are f5e_gemm_f32 / f5e_layernorm; these are the rest.  Per-row lengths
 * are DEVICE int [B] (NULL: every row is full).  No allocation, no synchronisation, nothing read back: all of it is
 * capturable. */

/* out[b][i] = (wav[b][i] - mean_b) / sqrt(var_b + 1e-5) for i < len[b], ZERO for len[b] <= i < S: mean and biased variance over
 * the row's valid samples (s3prl's F.layer_norm(wav, wav.shape)).  frames[b] (NULL to skip) = the frame count after the
 * n_conv <= 8 valid convolutions given by HOST arrays conv_kernels_host / conv_strides_host: n <- (n - k) / s + 1, 0 once
 * n < k.  mask (NULL to skip) f32 [B][t_mask] = t < frames[b], t_mask <= S.  Two launches: rows are cut into chunks of 4096
 * samples, one workgroup each; `partials` is scratch of f5e_wav_norm_partials(B, S) floats.  A chunk's statistics depend on
 * the valid samples only, so a padded row gives the bits of its B = 1 run. */
F5E_API int f5e_wav_norm(f5e_stream st, const float* wav, int ldw, const int* len, float* out, int ldo, float* partials,
                 int* frames, float* mask, int t_mask, const int* conv_kernels_host, const int* conv_strides_host,
                 int n_conv, int B, int S);
F5E_API int f5e_wav_norm_partials(int B, int S, unsigned long long* floats_out_host);

/* Layer 0 of the extractor in one pass: Conv1d(1 -> C, k = 10, stride 5, no padding; w f32 [C][10], bias [C] or NULL) +
 * LayerNorm over C (gamma, beta, eps 1e-5) + GELU(erf).  wav f32 [B][S] (row stride ldw) -> out[b][t][c], t < T0 <=
 * (S - 10) / 5 + 1, frames of a row C floats apart, rows out_bstride floats apart.  C <= 512. */
F5E_API int f5e_wavlm_conv0(f5e_stream st, const float* wav, int ldw, const float* w, const float* bias, const float* gamma,
                    const float* beta, float* out, long long out_bstride, int B, int S, int T0, int C);

/* out[r] = GELU(erf)(LayerNorm_C(x[r]) * gamma + beta), one pass, out may be x.  C <= 1024. */
F5E_API int f5e_layernorm_gelu(f5e_stream st, const float* x, int ldx, float* out, int ldo, const float* gamma,
                       const float* beta, long long rows, int C, float eps);

/* out[b][t] = x[b][t] + GELU(erf)(conv(x)[b][t] + bias) for t < frames[b], ZERO for frames[b] <= t < T.  conv: Conv1d(D, D,
 * k = taps, padding = pad, groups) evaluated at t = 0 .. T - 1 (for an even k with pad = k / 2 that is the reference's conv
 * with its last output frame dropped); frames outside [0, frames[b]) READ as zero whatever the buffer holds.  x, out f32
 * [B * T][D] (row strides ldx, ldo; no aliasing).  w_packed f32 [groups][taps][D / groups (oc)][D / groups (ic)] is the
 * weight-norm-folded weight.  v_mfma_f32_16x16x4_f32; D / groups a multiple of 4; 16-byte aligned operands. */
F5E_API int f5e_wavlm_posconv(f5e_stream st, const float* x, int ldx, const float* w_packed, const float* bias,
                      const int* frames, float* out, int ldo, int B, int T, int D, int groups, int taps, int pad);

/* gate[b][h][t] = a (b' const[h] - 1) + 2,  a = sigmoid(sum p[0:4]), b' = sigmoid(sum p[4:8]),
 * p = w_gate x[b][t][h dk : (h + 1) dk] + b_gate   (w_gate f32 [8][dk], b_gate [8], head_const [H]; x = the layer's NORMED
 * input, f32 [B * T][>= H dk]).  dk a multiple of 4, at most 128. */
F5E_API int f5e_wavlm_gate(f5e_stream st, const float* x, int ldx, const float* w_gate, const float* b_gate,
                   const float* head_const, float* gate, int B, int T, int H, int dk);

/* Self-attention with the gated relative-position bias computed on the fly (no [H][T][T] tensor exists):
 *   s[i][j] = scale q_i . k_j + gate[b][h][i] table[h][j - i + Tt - 1]   over keys j < kv_len[b]
 * q, k, v, out f32 [B * T][>= H dk]; gate f32 [B][H][T]; table f32 [H][2 Tt - 1], Tt >= T.  The wave tile of f5e_mha_f32.  A
 * query at or beyond kv_len[b] yields ZEROS.  dk in {16, 32, 64}. */
F5E_API int f5e_relbias_attn_f32(f5e_stream st, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                         float* out, int ldo, const float* gate, const float* table, int Tt, const int* kv_len, int B,
                         int T, int H, int dk, float scale);

/* ---------------------------------------------------------------- Whisper (csrc/whisper.hip) ----------------- */
/* Greedy Whisper recognition (reference infer/utils_infer.py:148-179, eval/utils_eval.py:631-672): the log-mel front-end, the
 * single-query cross-attention of a cached decoder step and the per-step greedy pick.  The convolution stem, the encoder and the
 * rest of the decoder step are f5e_im2col / f5e_gemm_f32 / f5e_layernorm / f5e_mha_f32 / f5e_attn_decode_f32 / f5e_text_gather.
 * fp32, no allocation, no synchronisation, nothing read back. */

/* WhisperFeatureExtractor on the device.  wav f32 [B][ldw], len DEVICE int [B] (NULL: the whole row): samples at or beyond
 * min(len[b], ldw) count as ZERO whatever the buffer holds, and the row is taken as hop * T samples long (the extractor's zero
 * padding to the chunk length; ldw may be shorter or longer).  Frame f < T covers [f hop - n_fft / 2, f hop + n_fft / 2) of that
 * row, reflect-padded at both ends (no edge repeat), times window f32 [n_fft] (periodic Hann); power re^2 + im^2 of the
 * n_fft / 2 + 1 bins by a direct DFT against twiddle f32 [n_fft][2] = (cos, sin)(2 pi i / n_fft); times fb f32
 * [n_fft / 2 + 1][n_mels] (Slaney); log10(max(., 1e-10)); max(x, rowmax_b - 8) with rowmax_b the maximum over all T * n_mels
 * values of utterance b; (x + 4) / 4.  (Frame T of the extractor's T + 1 is the one it drops: it is not computed.)
 * out f32 [B][T][n_mels], channels-last.  Two launches; partials: scratch of f5e_whisper_logmel_partials(B, T) floats (one
 * maximum per workgroup, folded in a fixed order: no float atomics).  F5E_ERR_UNSUPPORTED unless n_fft = 400, hop = 160 and
 * n_mels is 80 or 128; T >= 2. */
F5E_API int f5e_whisper_logmel_partials(int B, int T, unsigned long long* floats_out_host);
F5E_API int f5e_whisper_logmel(f5e_stream st, const float* wav, int ldw, const int* len, const float* window,
                       const float* twiddle, const float* fb, float* out, float* partials, int B, int T, int n_fft, int hop,
                       int n_mels);

/* Single-query cross-attention of a decoder step: for row r < R and head h, with u = r / rows_per_utt,
 *   out[r][h*dk + d] = sum_{j < n} softmax_j(scale * q[r][h*dk + :] . k[u][j][h*dk + :]) * v[u][j][h*dk + d],
 * n = kv_len[u] clamped to [0, Tk] (DEVICE int [R / rows_per_utt]) or Tk when kv_len is NULL (Whisper attends its zero-padded
 * frames: it passes NULL).  n = 0 yields zeros.  q, out [R][>= H*dk]; k, v [R / rows_per_utt][Tk][>= H*dk], computed once per
 * utterance; each operand has its own row stride.  One workgroup of four waves per (row, head): the waves split the keys, each
 * keeps a maximum, a sum and a context, merged through LDS.  Columns beyond H*dk of out are not touched.
 * dk = 16, 32, 64, 128 (else F5E_ERR_UNSUPPORTED); Tk <= 4096; R, H <= 65535; ldq, ldk multiples of 4 floats, q and k 16-byte
 * aligned. */
F5E_API int f5e_cross_attn_decode_f32(f5e_stream st, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                              float* out, int ldo, const int* kv_len, int R, int rows_per_utt, int Tk, int H, int dk,
                              float scale);

/* One greedy decoding step for R rows (transformers' SuppressTokensLogitsProcessor / SuppressTokensAtBeginLogitsProcessor +
 * argmax + the eos bookkeeping of generate), one workgroup per row over logits f32 [R][ld >= V] (only read).
 *   suppress i32 [n_sup]: classes at -inf at every step; begin_suppress i32 [n_beg]: also at -inf iff first_step != 0 (ids
 *   outside [0, V) are ignored); the pick is the LOWEST index among the equal maxima of what is left (0 if nothing is).
 *   A row with done[r] != 0 gets eos and stays done; otherwise the pick t goes to tokens[r][p + 1] and last[r] (contiguous, for
 *   the next f5e_text_gather), and t == eos sets done[r] = 1.  alive (one i32) = the rows with done[r] == 0 after the step.
 * Writes tokens[r][p + 1], last[r], done[r] (only from 0 to 1) and *alive -- nothing else.  tokens i32 [R][ld_tok >= p + 2].
 * V <= 262144, 0 <= eos < V. */
F5E_API int f5e_greedy_pick(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                    const int* begin_suppress, int n_beg, int first_step, int* tokens, int ld_tok, int* last, int* done,
                    int* alive, int R, int V, int p, int eos);

/* One step of Whisper's beam search for B utterances of K rows each (r = b K + i): transformers 5.15.0
 * GenerationMixin._beam_search with early_stopping = False and do_sample = False, its -1e9 sentinels replaced by flags.  K open
 * rows per utterance and a separate pool of at most K finished hypotheses ranked by score / length ** length_penalty (the wenet
 * rule of f5e_beam_step keeps finished rows INSIDE the beam instead).  n0 prompt tokens; step p feeds position p and chooses
 * column p + 1; cap = the largest total length.
 *   logits  f32 [B*K][ld_logits >= V], only read, ONCE per step: the raw decoder outputs of position p
 *   suppress i32 [n_sup], begin_suppress i32 [n_beg]: as f5e_greedy_pick; begin_suppress counts iff p + 1 == n0
 *   score   f32 [B*K] in/out: accumulated log-probabilities of the open rows.  Start: 0, -inf, ..., -inf per utterance
 *   hyp_in / anc_in  i32 [B*K][ld] the tables before the step, hyp_out / anc_out after it: DIFFERENT buffers, as f5e_beam_step
 *   last    i32 [B*K] out: hyp_out column p + 1, contiguous for the next embedding
 *   pool_hyp i32 [B][K][ld], pool_len i32 [B][K], pool_score f32 [B][K], pool_n i32 [B] (start 0): the pool, in/out, best
 *           first; entry s < pool_n[b] holds pool_len tokens (columns at or beyond are not defined)
 *   open    i32 [B] in/out, start 1: the utterance's pool still accepts.  alive i32 [B] out (rule 7)
 *   scratch f5e_whisper_beam_scratch(B, K, V) bytes, 4-byte aligned (no need to clear it)
 * Rules, per utterance:
 *  1. logp = (x - max) - log(sum exp(x - max)) over ALL V classes of the raw row (fp32); only then the classes of suppress (and
 *     of begin_suppress at the first step) become -inf: the normaliser includes them.
 *  2. Candidate value = score[r] + logp in fp32.
 *  3. The 2K largest FINITE candidates of the utterance's K V, in descending order; ties: lower row, then lower class.  A
 *     candidate is hit iff its class is eos or p + 2 >= cap.
 *  4. New rows 0..K-1 = the first K candidates that are not hit, in order: the parent's hyp columns 0..p plus the class at
 *     column p + 1, the parent's anc columns < p plus the parent's GLOBAL row at column p, score = the value, last = the class.
 *     Rows beyond the candidates there are keep their own prefix, get eos at column p + 1 and score -inf.
 *  5. If open[b]: every hit candidate AMONG THE FIRST K of the 2K enters the pool with score value / (p + 2 - n0) **
 *     length_penalty, its p + 2 tokens and length p + 2.  The pool keeps the K best in descending order; an old entry goes
 *     before a newcomer of equal score, newcomers keep candidate order.  Hit candidates ranked K..2K-1 neither run nor enter.
 *  6. If the pool holds K entries: open[b] &= score_new[row 0] / (p + 2 - n0) ** length_penalty > pool_score[K-1].
 *  7. alive[b] = open[b] && not every candidate was hit.
 * A closed utterance keeps updating its rows; its pool is frozen.  The answer is pool entry 0.
 * Two launches.  The first, one workgroup per (row, chunk of 8192 classes), stages the chunk in LDS and leaves its maximum, its
 * sum of exponentials and its 2K largest unsuppressed (value, class) in scratch; the second, one workgroup per utterance, folds
 * the chunks in ascending order, selects and applies the rules.  No float atomics; the result is deterministic.
 * Containment: columns > p + 1 of hyp_out, columns > p of anc_out, the input tables, the logits, pool slots that do not change
 * and scratch beyond the queried size are untouched.
 * Limits: 1 <= K <= 16 and V <= 262144 (else F5E_ERR_UNSUPPORTED), 2K <= V, 0 <= eos < V, n0 >= 1, n0 - 1 <= p, ld >= p + 2,
 * cap <= ld, B <= 65535.  No allocation, no synchronisation. */
F5E_API int f5e_whisper_beam_scratch(int B, int K, int V, unsigned long long* bytes_out_host);
F5E_API int f5e_whisper_beam_step(f5e_stream st, const float* logits, long long ld_logits, const int* suppress, int n_sup,
                          const int* begin_suppress, int n_beg, float* score, const int* hyp_in, const int* anc_in, int* hyp_out,
                          int* anc_out, int ld, int* last, int* pool_hyp, int* pool_len, float* pool_score, int* pool_n,
                          int* open, int* alive, void* scratch, unsigned long long scratch_bytes, int B, int K, int V, int p,
                          int n0, int cap, int eos, float length_penalty);

/* Whisper's timestamp rules (transformers 5.15.0 WhisperTimeStampLogitsProcessor, run after the two suppress processors) for
 * decoding WITH timestamp tokens.  ts_begin = no_timestamps + 1; a class >= ts_begin is a timestamp, every other one is text.
 * The generated tokens of row r are h = tokens[r][n0 .. p] (none at the first step p = n0 - 1).  Banned, besides the classes of
 * suppress (and of begin_suppress iff p + 1 == n0):
 *  1. <|notimestamps|> itself.
 *  2. h ends with a timestamp and the token before it is a timestamp or absent: every timestamp.
 *  3. h ends with a timestamp after a text token: the classes [0, eos) -- [eos, ts_begin) stay, as in the processor.
 *  4. With T the last timestamp of h: the timestamps below T in state 3, the timestamps up to and including T otherwise.
 *  5. First step: all text; with max_initial >= 0 also the timestamps above ts_begin + max_initial (-1: no such limit).
 *  6. If log-sum-exp over the timestamps still allowed > the maximum over the text still allowed: all text.  (The processor
 *     compares log-probabilities; their normaliser is common to both sides.)  NaN and infinite logits count as banned.
 * f5e_whisper_ts_pick: one greedy step under these rules, as f5e_greedy_pick otherwise (lowest index among equal maxima, 0 if
 *   nothing is allowed; done rows get eos; tokens[r][p + 1], last[r], done[r] 0 -> 1, *alive), and for a row that was not done
 *   sum_logp[r] += (x[pick] - M) - log(sum over the allowed classes of exp(x - M)), M their maximum: the log-softmax of the
 *   processed scores at the pick (the closing eos counts).  One workgroup per row reads the logits once: per lane a running
 *   maximum / first index / sum of exponentials for the timestamps and for the text, folded by shuffles and through LDS in a
 *   fixed order.  Writes nothing else; the logits are only read.
 * f5e_whisper_ts_rule: the same pass, leaving only the row's rule descriptor desc[r][0..4) = {text ban: 0 none, 1 [0, eos),
 *   2 [0, ts_begin); lo; hi (the timestamps allowed are [lo, hi], none if lo > hi); 0}.
 * f5e_whisper_beam_step_ts: f5e_whisper_beam_step with the rules: f5e_whisper_ts_rule on hyp_in into desc i32 [B*K][4] (the
 *   caller's buffer), then the chunk launch strikes the banned classes after the suppressed ones (rule 1 of the beam step is
 *   unchanged: the normaliser covers all V raw classes).  Three launches.
 * Limits: 2 <= V <= 262144, 0 <= eos <= no_timestamps < V - 1, n0 >= 1, p >= n0 - 1, ld_tok >= p + 2, max_initial >= -1; the
 * beam's own limits as above. */
F5E_API int f5e_whisper_ts_pick(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                        const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int* last, int* done, int* alive,
                        float* sum_logp, int R, int V, int p, int n0, int eos, int no_timestamps, int max_initial);
F5E_API int f5e_whisper_ts_rule(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                        const int* begin_suppress, int n_beg, const int* tokens, int ld_tok, int* desc, int R, int V, int p,
                        int n0, int eos, int no_timestamps, int max_initial);
F5E_API int f5e_whisper_beam_step_ts(f5e_stream st, const float* logits, long long ld_logits, const int* suppress, int n_sup,
                             const int* begin_suppress, int n_beg, float* score, const int* hyp_in, const int* anc_in,
                             int* hyp_out, int* anc_out, int ld, int* last, int* pool_hyp, int* pool_len, float* pool_score,
                             int* pool_n, int* open, int* alive, void* scratch, unsigned long long scratch_bytes, int B, int K,
                             int V, int p, int n0, int cap, int eos, float length_penalty, int no_timestamps, int max_initial,
                             int* desc);

/* f5e_whisper_sample_pick: f5e_whisper_ts_pick with a draw in place of the argmax (temperature fallback).  The noise
 * is a pure function of counters:
 *   w   = Philox4x32-10(counter = (i >> 2, p, serial[r], row_key[r]), key = (seed & 0xffffffff, seed >> 32)), class i uses word
 *         i & 3 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl increments 0x9E3779B9 / 0xBB67AE85);
 *   u_i = ((w >> 8) + 0.5) * 2^-24, strictly inside (0, 1);   g_i = -log(-log(u_i));
 *   pick = the lowest index among the maxima of x_i / temperature + g_i over the allowed classes (Gumbel-max: a draw from
 *         softmax(x / temperature) over them), 0 if nothing is allowed.
 * Rules 1-6 are decided on the raw logits (the temperature warper runs after the Whisper processors), and sum_logp gains the
 * T = 1 log-softmax of the processed scores at the pick, (x[pick] - M) - log(sum over the allowed classes of exp(x - M)), as in
 * f5e_whisper_ts_pick.  fp32: x / temperature is one division, g uses the accurate logf / log1pf (the upper half of u goes
 * through 1 - u, which fp32 holds exactly there), the sum is one addition.  no_timestamps = -1: no timestamp rules (every class
 * is text; max_initial is ignored).  row_key, serial: DEVICE i32 [R].  One workgroup per row, one pass, the logits are read once;
 * writes tokens[r][p + 1], last, done (0 -> 1), *alive and sum_logp, nothing else.
 * Limits: those of f5e_whisper_ts_pick (or no_timestamps = -1), and a finite temperature > 0. */
F5E_API int f5e_whisper_sample_pick(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                            const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int* last, int* done, int* alive,
                            float* sum_logp, int R, int V, int p, int n0, int eos, int no_timestamps, int max_initial,
                            float temperature, unsigned long long seed, const int* row_key, const int* serial);

/* ---------------------------------------------------------------- Whisper word timestamps (csrc/whisper_align.hip) */
/* Token times from the cross-attention of a few "alignment heads" (transformers 5.15.0 generation_whisper.py:
 * _extract_token_timestamps, _median_filter, _dynamic_time_warping with num_frames given), for one utterance with the
 * hypothesis tokens[0..n), n0 of them the prompt, `frames` mel frames, M = frames / 2 encoder positions clamped to 1 .. 1500,
 * alignment heads (decoder layer, head) and an odd filter width w (7):
 *  1. Row t of a head = softmax over ALL Tk encoder keys of the scaled scores of the query produced when the token at position
 *     n0 + t is fed; only its first M columns are kept.  t = 0 .. N - 1 with N = n - n0 - 1: the last token is never fed (with
 *     "include_last", OpenAI's rule, N = n - n0).
 *  2. Per head and column j: mean and POPULATION standard deviation over the N rows; z = (p - mean) / std.
 *  3. Median of width w along j, reflect padding of w / 2 (no edge repeat); rows stay unfiltered when M <= w / 2.
 *  4. C[t][j] = -(mean over the heads of the filtered z), fp32.
 *  5. cost fp32 [N + 1][M + 1] = +inf except cost[0][0] = 0.  With c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]:
 *     diagonal if c0 < c1 && c0 < c2, else up if c1 < c0 && c1 < c2, else left (STRICT comparisons: every tie goes left);
 *     cost[i][j] = C[i-1][j-1] + the chosen cost, ONE fp32 addition (the reference adds a float64 that holds an fp32 value to an
 *     fp32 and rounds to fp32: the same number).
 *  6. Backtrace from (N, M); row 0 forces left, column 0 forces up.  first[t] = the column at which the path enters row t (the
 *     smallest j - 1 over its cells (t + 1, j)); the time of token n0 + t is first[t] * 0.02 s.
 *  7. N = 0: no row, every time 0.  N = 1: time 0 (the reference gets there through NaNs; here nothing is NaN).  A column whose
 *     standard deviation is 0 (every column when N = 1) gives NaN in the reference; HERE ITS z IS 0, a defined result.
 * fp32, no allocation, no synchronisation, nothing read back, no atomics; lengths are DEVICE int32; all of it is capturable. */

/* Rule 1 for the heads of ONE layer: for row r < R, u = r / rows_per_utt and s < n_sel with h = heads[s] (DEVICE int [n_sel]),
 *   probs[r * stride_row + s * stride_sel + j] = softmax_{all Tk keys}(scale * q[r][h*dk + :] . k[u][:][h*dk + :])[j]
 * for j < min(m_len[u], M_cap, Tk) (m_len: DEVICE int [R / rows_per_utt], NULL: Tk; M_cap >= 1: the columns the caller has room
 * for).  Strides in floats; the caller puts a token
 * position and a head's place among all alignment heads into the `probs` pointer.  Columns at or beyond that bound, and everything
 * of a head index outside [0, H), are NOT written.  q [R][ldq >= H*dk]; k [R / rows_per_utt][Tk][ldk >= H*dk].  One workgroup
 * of four waves per (row, selected head); maximum and sum are folded over the waves in a fixed order.  A launch of its own:
 * f5e_cross_attn_decode_f32 is unchanged.  dk = 16, 32, 64, 128 (else F5E_ERR_UNSUPPORTED); Tk <= 4096; R, H, n_sel <= 65535;
 * ldq, ldk multiples of 4 floats, q and k 16-byte aligned (else F5E_ERR_BAD_SHAPE). */
F5E_API int f5e_cross_attn_probs_f32(f5e_stream st, const float* q, int ldq, const float* k, int ldk, const int* heads,
                             int n_sel, const int* m_len, int M_cap, float* probs, long long stride_row, long long stride_sel,
                             int R, int rows_per_utt, int Tk, int H, int dk, float scale);

/* Rules 2-4.  probs f32 [B][n_sel][N_cap][ld >= M_cap] (only read), n_rows / m_len DEVICE int [B] (clamped to [0, N_cap] /
 * [0, M_cap]) -> C f32 [B][N_cap][ldc >= M_cap].  Cells outside (n_rows[b], m_len[b]) are NOT written.  One launch: a workgroup
 * owns 64 columns (+ w / 2 on each side) of an utterance, keeps mean and std of every (head, column) in LDS, and takes the
 * median by rank counting.  1 <= n_sel <= 64 and width odd in 1 .. 15 (else F5E_ERR_UNSUPPORTED); 1 <= N_cap <= 448,
 * 1 <= M_cap <= 4096, B <= 65535 (else F5E_ERR_BAD_SHAPE). */
F5E_API int f5e_dtw_cost_f32(f5e_stream st, const float* probs, int ld, const int* n_rows, const int* m_len, float* C, int ldc,
                     int B, int n_sel, int N_cap, int M_cap, int width);

/* Rules 5-7.  C f32 [B][N_cap][ldc >= M_cap] (only read), n_rows / m_len DEVICE int [B] -> first i32 [B][N_cap]: first[b][t]
 * for t < n_rows[b], -1 beyond.  An utterance whose lengths are not in 1 .. N_cap / 1 .. M_cap gets a whole row of -1.  One
 * workgroup per utterance walks the anti-diagonals i + j with one barrier each: thread i owns row i, keeps cost[i][j-1] and
 * cost[i-1][j-1] in registers and reads cost[i-1][j] from a double-buffered LDS row; two trace bits per cell go to `workspace`
 * (f5e_dtw_workspace_bytes(B, N_cap, M_cap) bytes, 4-byte aligned, no need to clear it; nothing beyond that size is touched);
 * one thread walks the backtrace.  1 <= N_cap <= 448 and 1 <= M_cap <= 4096 (else F5E_ERR_UNSUPPORTED); B <= 65535. */
F5E_API int f5e_dtw_workspace_bytes(int B, int N_cap, int M_cap, unsigned long long* bytes_out_host);
F5E_API int f5e_dtw_path(f5e_stream st, const float* C, int ldc, const int* n_rows, const int* m_len, int* first,
                 void* workspace, unsigned long long workspace_bytes, int B, int N_cap, int M_cap);

/* ---- Whisper decoder prefill (csrc/whisper_prefill.hip): a prompt of U positions per row in ONE pass per layer.
 *
 * Causal self-attention of positions 0 .. U-1 of R rows against themselves, which also files their keys and values:
 *   qkv     f32 [R*U][ld_qkv >= 3*H*dk]: the fused projection q | k | v, row r*U + i = position i of row r
 *   kc, vc  the layer's caches as f5e_attn_decode_f32 takes them: element (r, j, c) at r*row_stride + j*pos_stride + c
 *   begin   i32 [R] on the device or NULL (all 0): row r is left-padded by begin[r] positions (clamped to [0, U])
 *   out     f32 [R*U][ldo >= H*dk]
 * out[r*U + i][h*dk + d] = sum_{j = begin[r] .. i} softmax_j(scale * q_i . k_j) * v_j[d]; a query i < begin[r] yields zeros.
 * Slots [r][0 .. U-1] of kc / vc receive the k / v columns of qkv bit for bit (the padded positions too: nobody reads them);
 * no other byte of the caches is written, and keys / values are read from qkv, never from the caches.  The wave tile of
 * f5e_mha_f32 (16 queries per wave on v_mfma_f32_16x16x4_f32); the tile that owns 16 positions of a head stores their k and v.
 * Limits: 1 <= U <= Umax <= 4096; dk = 16, 32, 64, 128; R, H <= 65535; every stride a multiple of 4 floats; qkv, kc, vc and out
 * 16-byte aligned.  Refusals happen before the launch.  No allocation, no synchronisation. */
F5E_API int f5e_attn_prefill_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                         int pos_stride, const int* begin, float* out, int ldo, int R, int U, int Umax, int H, int dk,
                         float scale);
/* f5e_attn_decode_f32 for a row whose first begin[r] positions are padding: keys / values begin[r] .. p (begin clamped to
 * [0, p]).  begin i32 [R] on the device; NULL runs f5e_attn_decode_f32 itself, and zeros give its bits.  Everything else
 * (slot [r][p], the ancestry table, the limits) as there. */
F5E_API int f5e_attn_decode_from_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                             int pos_stride, const int* anc, int ld_anc, const int* begin, float* out, int ldo, int R, int Umax,
                             int H, int dk, int p, float scale);
/* out[r][u] = emb[ids[r][u]] + pos[max(p0 + u - begin[r], 0)]: ids i32 [R][U], begin i32 [R] or NULL, emb f32 [table_rows][D],
 * pos f32 [max_pos][D], out f32 [R][U][D] (all contiguous, D a multiple of 4, 16-byte aligned).  U = 1 with p0 = p is the decode
 * step's form.  An id outside the table is clamped (the host refuses it where it knows the ids); p0 + U <= max_pos. */
F5E_API int f5e_whisper_embed(f5e_stream st, const int* ids, const int* begin, const float* emb, const float* pos, float* out,
                      int R, int U, int D, int p0, int max_pos, int table_rows);

/* ---- Whisper speculative decoding (csrc/whisper_append.hip, csrc/gemm_f32_skinny.hip): a draft model proposes U tokens with
 * cheap steps, the large model checks them in ONE pass per layer and keeps the longest prefix it agrees with plus its own next
 * token.
 *
 * f5e_attn_append_f32: causal self-attention of the U NEW positions p0 .. p0+U-1 of R rows behind an existing cache.  qkv f32
 * [R*U][ld_qkv >= 3*H*dk] (row r*U + u = position p0 + u of row r), kc / vc / begin / out as f5e_attn_prefill_f32 takes them.
 * Query u of row r sees the cached keys begin[r] .. p0-1, read from kc / vc (16-key tiles from begin[r] & ~15, masked at both
 * edges, no causal mask), and the new keys 0 .. u of its own row, read from qkv and never from the caches (causal mask); one
 * online softmax runs across both.  A query whose position lies below begin[r] (clamped to [0, p0 + U]) yields exact zeros.
 * Slots [r][p0 .. p0+U-1] of kc / vc receive the k / v columns of qkv bit for bit; the launch reads only slots below p0 and
 * writes only those, so it reads nothing that it writes.  p0 = 0 computes what f5e_attn_prefill_f32 computes.  The wave tile,
 * the cache strides (the beam view included) and the limits are f5e_attn_prefill_f32's; p0 < 0 and p0 + U > Umax are refused. */
F5E_API int f5e_attn_append_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                        int pos_stride, const int* begin, float* out, int ldo, int R, int U, int Umax, int H, int dk, int p0,
                        float scale);
/* f5e_whisper_verify: for every row r and every j in 0 .. U, the pick that f5e_greedy_pick (no_timestamps = -1) or
 * f5e_whisper_ts_pick would make at position p + j on logits row r*(U+1) + j with the generated tokens hist[r][n0 .. p+j]:
 *   logits  f32 [R*(U+1)][ld >= V], only read once
 *   hist    i32 [R][ld_hist >= p + U + 1]: the final tokens up to column p, the drafts in columns p+1 .. p+U
 *   cand    i32 [R][U+1], logp f32 [R][U+1]: the pick, and the sum_logp increment of f5e_whisper_ts_pick (0 without rules)
 * begin_suppress counts iff p + j + 1 == n0.  One workgroup per (r, j); picks and increments are bit-equal to the single-step
 * kernels on the same inputs (one body, csrc/whisper_pick.h).  Rows that are done are computed like the others.
 * Limits: R <= 65535, U >= 0, 2 <= V <= 262144, n0 >= 1, p >= n0 - 1; with rules those of f5e_whisper_ts_pick. */
F5E_API int f5e_whisper_verify(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                       const int* begin_suppress, int n_beg, const int* hist, int ld_hist, int* cand, float* logp, int R, int U,
                       int V, int p, int n0, int eos, int no_timestamps, int max_initial);
/* f5e_whisper_accept: one launch after f5e_whisper_verify.  For a row that is not done, m[r] = the number of leading j < U with
 * cand[r][j] == hist[r][p+1+j], counting no further than a cand that is eos.  The common advance a = min over the open rows of
 * m[r] + 1 (1 .. U + 1; 1 when no row is open).  Every row gets tokens[r][p+1 .. p+a]: an open row cand[r][0 .. a-1], from its
 * first eos on eos (done 0 -> 1); a done row eos.  last[r] = tokens[r][p+a]; sum_logp[r] (may be NULL) gains the logp of the
 * kept picks one by one, the closing eos included, nothing after it and nothing for done rows; *alive = rows still open;
 * adv[0] = a.  hist is put right: tokens on columns p+1 .. p+a, eos on p+a+1 .. p+U.  Columns of tokens beyond p + a are not
 * touched.  tokens and hist rows hold at least p + U + 2 columns; U >= 1. */
F5E_API int f5e_whisper_accept(f5e_stream st, const int* cand, const float* logp, int* hist, int ld_hist, int* tokens, int ld_tok,
                       int* last, int* done, int* alive, float* sum_logp, int* adv, int R, int U, int p, int eos);
/* f5e_gemm_f32_skinny: out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) + addend[m][n] for 1 <= M <= 16 rows, fp32: the GEMM of a
 * verify pass, which is one read of W.  W is cut into tiles of 16 rows and, where N is small, K into KS slices, so that the read
 * is spread over every CU; the K ranges are summed in a fixed order (through LDS inside a workgroup, through `workspace` and a
 * second launch across workgroups): no floating-point atomics, a launch is bit-reproducible, and a row's result does not
 * depend on M.  act: F5E_ACT_NONE or F5E_ACT_GELU_ERF; bias [N] and addend [M][ld_add] may be NULL; addend may alias out.
 * K % 4 == 0, lda and ldw multiples of 4, A and W 16-byte aligned; ldo and ld_add are free.  A must not alias out.
 * workspace: f5e_gemm_f32_skinny_workspace(N, K) bytes (0 when K is not split; host arithmetic on N, K and the CU count), 16-byte
 * aligned.  M = 17 and the rest are refused before the launch. */
F5E_API int f5e_gemm_f32_skinny_workspace(int N, int K, unsigned long long* bytes_out_host);
F5E_API int f5e_gemm_f32_skinny(f5e_stream st, const float* A, int lda, const float* W, int ldw, const float* bias, int act,
                        const float* addend, int ld_add, float* out, int ldo, void* workspace,
                        unsigned long long workspace_bytes, int M, int N, int K);

/* ---- Whisper's decode step with the position on the device (csrc/whisper_step.hip): what a hipGraph of ONE step needs so that
 * it can be captured once and replayed per token.  Everything that changes from token to token is read from the
 * step record `rec`, DEVICE i32 [8], 16-byte aligned:
 *   rec[0] p (the position fed; the pick writes token column p + 1), rec[1] n0 (the prompt length; first_step = p + 1 == n0),
 *   rec[2], rec[3] the low / high word of the sampled pick's seed, rec[4] the bits of its fp32 temperature, rec[5..7] reserved.
 * The arithmetic is that of the host-position entry points (one body each), so the bits are theirs.  Every kernel clamps what
 * it reads from the record to the extents of its launch, the grids do not depend on it, and no kernel waits for another
 * workgroup.  p is advanced by exactly one thread: thread 0 of the one-workgroup launch that follows a pick.
 *
 * f5e_attn_decode_dev_f32: f5e_attn_decode_f32 (begin NULL) / f5e_attn_decode_from_f32 without an ancestry table, at
 * p = clamp(rec[0], 0, P - 1), P = the cached positions per row.  Grid (H, R).  Limits as there. */
F5E_API int f5e_attn_decode_dev_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                            int pos_stride, const int* begin, float* out, int ldo, int R, int P, int H, int dk, const int* rec,
                            float scale);
/* out[r] = emb[last[r]] + pos[p - begin[r]] with p = max(rec[0], 0), begin[r] clamped to [0, p] (NULL: 0) and the row of pos
 * to the table: f5e_whisper_embed with U = 1 (and f5e_text_gather with one position row).  last i32 [R], out f32 [R][D]. */
F5E_API int f5e_whisper_embed_dev(f5e_stream st, const int* last, const int* begin, const float* emb, const float* pos, float* out,
                          int R, int D, const int* rec, int max_pos, int table_rows);
/* f5e_greedy_pick / f5e_whisper_ts_pick / f5e_whisper_sample_pick at p = clamp(rec[0], 0, n_tok - 2), n_tok = the columns of a
 * token row (ld_tok its stride), n0 = rec[1] (the ruled picks: clamped to [1, p + 1]), begin_suppress counted iff p + 1 == n0,
 * the seed and the temperature from the record; then one workgroup writes *alive and rec[0] += 1.  Nothing else of the record
 * is written. */
F5E_API int f5e_greedy_pick_dev(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                        const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int n_tok, int* last, int* done, int* alive,
                        int R, int V, int* rec, int eos);
F5E_API int f5e_whisper_ts_pick_dev(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                            const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int n_tok, int* last, int* done,
                            int* alive, float* sum_logp, int R, int V, int* rec, int eos, int no_timestamps, int max_initial);
F5E_API int f5e_whisper_sample_pick_dev(f5e_stream st, const float* logits, long long ld, const int* suppress, int n_sup,
                                const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int n_tok, int* last, int* done,
                                int* alive, float* sum_logp, int R, int V, int* rec, int eos, int no_timestamps, int max_initial,
                                const int* row_key, const int* serial);

/* ---- The fp32 GEMM family with a 16-bit weight operand (csrc/gemm_f32_w16.hip, csrc/w_load.h; DESIGN 4o "16-bit weights").
 * W is fp16 (wtype = F5E_W_FP16) or bf16 (F5E_W_BF16), row-major [N][ldw] with ldw in ELEMENTS, 8-byte aligned, ldw % 4 == 0.
 * It is widened to fp32 in registers on load (bf16: the 16 bits become the high half of the float; fp16: the hardware
 * convert, subnormals kept); activations, accumulation, bias, epilogue and outputs are fp32 as in the fp32 entry points, whose
 * kernel bodies these share.  Widening is exact and the summation order is the fp32 kernel's, so each call gives THE BITS of
 * its fp32 sibling on the (16-byte aligned) widened copy of W, reading half the bytes of W.  Every other argument, limit and
 * refusal is the sibling's; another wtype is refused.
 *
 * f5e_gemm_f32_w16_skinny (+ _workspace, which answers what f5e_gemm_f32_skinny_workspace answers): 1 <= M <= 16 rows.
 * f5e_gemm_f32_w16: every epilogue term of f5e_gemm_f32, a_rows / add_rows broadcast, a_act, out and / or out_bf16.
 * f5e_whisper_embed_w16 / _dev: f5e_whisper_embed / f5e_whisper_embed_dev with a 16-bit token table emb [table_rows][D] (8-byte
 * aligned); pos stays fp32. */
F5E_API int f5e_gemm_f32_w16_skinny_workspace(int N, int K, unsigned long long* bytes_out_host);
F5E_API int f5e_gemm_f32_w16_skinny(f5e_stream st, const float* A, int lda, const void* W, int ldw, int wtype, const float* bias,
                            int act, const float* addend, int ld_add, float* out, int ldo, void* workspace,
                            unsigned long long workspace_bytes, int M, int N, int K);
F5E_API int f5e_gemm_f32_w16(f5e_stream st, const float* A, int lda, int a_rows, int a_act, const void* W, int ldw, int wtype,
                     const float* bias, int act, const float* ch_scale, const float* addend, int ld_add, int add_rows,
                     const float* row_scale, float* out, int ldo, void* out_bf16, int ldo_bf16, int M, int N, int K);
F5E_API int f5e_whisper_embed_w16(f5e_stream st, const int* ids, const int* begin, const void* emb, int wtype, const float* pos,
                          float* out, int R, int U, int D, int p0, int max_pos, int table_rows);
F5E_API int f5e_whisper_embed_w16_dev(f5e_stream st, const int* last, const int* begin, const void* emb, int wtype,
                              const float* pos, float* out, int R, int D, const int* rec, int max_pos, int table_rows);

/* ---------------------------------------------------------------- UTMOS (csrc/utmos.hip) ---------------------- */
/* The UTMOS predictor (utmos22_strong, reference eval/eval_utmos.py): a wav2vec2-base upstream (group-norm feature extractor,
 * post-LayerNorm encoder), a BiLSTM over its frames and a per-frame score averaged per utterance.  The strided convolutions 1-6,
 * the projections, the attention and the feed-forward are f5e_gemm_f32 / f5e_layernorm / f5e_wavlm_posconv / f5e_mha_f32; these
 * are the rest.  fp32, channels-last, per-row lengths DEVICE int [B] (NULL: every row is full).  No allocation, no
 * synchronisation, nothing read back, no floating-point atomics (every reduction runs in a fixed order): all of it is
 * capturable, and a replay gives the bits of the eager run. */

/* Layer 0 of the group-norm extractor: out[b][t][c] = GELU(erf)(gamma[c] (y - mean_bc) / sqrt(var_bc + eps) + beta[c]) with
 * y = Conv1d(1 -> C, k = 10, stride 5, no padding; w f32 [C][10], bias [C] or NULL) of row b of wav f32 [B][S] (row stride ldw)
 * and mean / biased variance of channel c over the T0_b = (len[b] - 10) / 5 + 1 frames of ITS OWN row (0 below 10 samples; len
 * clamped to [0, S]), so row b of a padded batch equals its B = 1 run whatever the padding holds.  Frames t in [T0_b, T0),
 * T0 = (S - 10) / 5 + 1, are written as ZERO; frames of `out` at or beyond T0 are not touched.  Frames of a row are C floats
 * apart, rows out_bstride >= T0 C floats.  Two launches, both recompute the 10 taps: per-chunk (mean, M2) of 256 frames (the
 * count follows from T0_b), merged per channel in ascending order by Chan's pairwise update in double (never E[x^2] - mean^2),
 * then the apply pass; T0_b = 1 gives GELU(beta) exactly.  `partials`: scratch of f5e_w2v_conv0_gn_partials(B, S, C) floats.
 * Also writes what f5e_wav_norm does for the layers above: frames[b] (NULL to skip) = the frame count of len[b] samples after the
 * n_conv <= 8 valid convolutions of the HOST arrays, and mask (NULL to skip) f32 [B][t_mask] = t < frames[b], t_mask <= S. */
F5E_API int f5e_w2v_conv0_gn_partials(int B, int S, int C, unsigned long long* floats_out_host);
F5E_API int f5e_w2v_conv0_gn(f5e_stream st, const float* wav, int ldw, const float* w, const float* bias, const float* gamma,
                     const float* beta, const int* len, float* partials, float* out, long long out_bstride, int* frames,
                     float* mask, int t_mask, const int* conv_kernels_host, const int* conv_strides_host, int n_conv, int B,
                     int S, int C, float eps);

/* The recurrence of a single-layer LSTM, ND = 1 (forward) or 2 (bidirectional) directions, PyTorch gate order i, f, g, o, zero
 * initial state.  xg f32 [B * T][>= ND 4 H] (row stride ldxg) holds x W_ih^T + b_ih + b_hh of both directions, column
 * d 4 H + gate H + unit (one f5e_gemm_f32 beforehand); w_hh_packed f32 [ND][H (unit)][H / 64][64][4 (gate)] with
 * w_hh_packed[d][u][j][l][g] = W_hh[d][g H + u][64 j + l], 16-byte aligned; out f32 [B][T][ND H]; cell: scratch f32 [ND][B][H]
 * (no need to clear it).  Packed-sequence semantics: direction 0 walks t = 0 .. len[b] - 1, direction 1 walks len[b] - 1 .. 0,
 * so a padded row equals its own B = 1 run; out[b][t >= len[b]] = 0 and rows of xg at or beyond len[b] are never read (len
 * clamped to [0, T]).  T launches, one per time step, both directions and all rows in each; a workgroup owns 4 hidden units with
 * all four gate rows, reads h of the neighbouring step from `out`, and is the only writer of its cells.  No workgroup waits on
 * another: the stream order is the only ordering.  expf / tanhf.  H a multiple of 64 up to 1024, B <= 16, 1 <= T <= 4096. */
F5E_API int f5e_lstm_f32(f5e_stream st, const float* xg, long long ldxg, const float* w_hh_packed, const int* len, float* out,
                 float* cell, int B, int T, int H, int ND);

/* frame[b][t] = hid[b T + t][0 .. F) . w2 + b2[0]  (hid f32 [B * T][>= F], row stride ldh; b2 DEVICE f32 [1] or NULL) and
 * out[b] = scale * mean_{t < n_b} frame[b][t] + offset, n_b = frames[b] clamped to [0, T] (NULL: T; n_b = 0 gives offset).
 * frame_scores (NULL to skip) f32 [B][T], ZERO at t >= n_b.  One workgroup per row, sums in a fixed order. */
F5E_API int f5e_score_mean(f5e_stream st, const float* hid, long long ldh, const float* w2, const float* b2, const int* frames,
                   float* frame_scores, float* out, int B, int T, int F, float scale, float offset);

/* ---------------------------------------------------------------- Paraformer (csrc/paraformer.hip) ------------ */
/* funasr's paraformer-zh, the Chinese recogniser of the reference's WER (eval/utils_eval.py:472-482): the LFR + CMVN front
 * behind f5e_kaldi_fbank, the FSMN memory block of the SANM attention, the CIF predictor and the pick of the non-autoregressive
 * decoder.  The projections, norms, convolutions-as-GEMM and attentions are f5e_gemm_f32 / f5e_layernorm / f5e_im2col /
 * f5e_mha_f32.  fp32, channels-last, per-row lengths DEVICE int [B] clamped to [0, T] (NULL: every row is full).  No
 * allocation, no synchronisation, nothing read back, no atomics: capturable, a replay gives the bits of the eager run.  Every
 * product and sum is rounded on its own (no fused multiply-add). */

/* Low frame rate + CMVN + the encoder's input scale and position table in one pass, each step rounded separately:
 *   out[b][i][j n_mels + c] = ((fbank[b][f][c] + shift[k]) * scale[k]) * xscale + pos[i][k],  k = j n_mels + c,
 *   f = clamp(n i + j - (m - 1) / 2, 0, T_b - 1)   for i < T'_b = ceil(T_b / n), ZERO for T'_b <= i < Tp,
 * i.e. (m - 1) / 2 copies of frame 0 in front, the last frame repeated behind.  fbank f32 [B][T][n_mels]; shift, scale f32
 * [m n_mels]; pos f32 [pos_rows >= Tp][m n_mels] or NULL; out f32 [B][Tp][m n_mels], Tp >= ceil(T / n).  T_b = count[b]
 * (hop == 0: frames) or kaldi's snip_edges frame count of count[b] samples, 0 below win, else 1 + (count[b] - win) / hop
 * (hop > 0); NULL: T.  frames_out (NULL to skip) int [B] receives T'_b.  No frame at or beyond T_b is read. */
F5E_API int f5e_lfr_cmvn_f32(f5e_stream st, const float* fbank, const int* count, int win, int hop, const float* shift,
                     const float* scale, const float* pos, int pos_rows, float* out, int* frames_out, int B, int T, int Tp,
                     int n_mels, int m, int n, float xscale);

/* The masked depthwise memory block (FSMN) of the SANM attention and of the decoder:
 *   out[b][t][c] = sum_{j < K} w_t[j][c] x[b][t + j - left][c] + x[b][t][c]  (+ addend[b][t][c])   for t < len[b],
 *   out[b][t][c] = addend[b][t][c] (or 0 without an addend)                                        for t >= len[b],
 * a tap outside [0, len[b]) contributing nothing: it never reads a frame at or past the row's length nor the neighbouring batch
 * row.  x, addend, out f32 [B * T][>= C] with their own row strides (x may be the v third of a q | k | v buffer); w_t f32 [K][C]
 * (Conv1d weight [C][1][K] transposed).  out may be addend itself, not x.  C and the strides multiples of 4, operands 16-byte
 * aligned, 1 <= K <= 256, 0 <= left < K. */
F5E_API int f5e_fsmn_f32(f5e_stream st, const float* x, int ldx, const float* w_t, const int* len, const float* addend, int ld_add,
                 float* out, int ldo, int B, int T, int C, int K, int left);

/* x[b][t][0 .. C) = 0 for t >= len[b], in place; x f32 [B * T][ldx >= C]. */
F5E_API int f5e_mask_rows_f32(f5e_stream st, float* x, int ldx, const int* len, int B, int T, int C);

/* CIF weights: alpha[b][t] = max(sigmoid(logits[b T + t]) * smooth - noise, 0) for t < len[b], `tail` at t = len[b] (the tail
 * step), 0 beyond; alpha f32 [B][ld_alpha >= T + 1], logits one float every ld_logits.  n_out int [B] = floor(sum_t alpha[b][t]),
 * summed in double in a fixed order. */
F5E_API int f5e_cif_alpha_f32(f5e_stream st, const float* logits, int ld_logits, const int* len, float* alpha, int ld_alpha,
                      int* n_out, int B, int T, float smooth, float noise, float tail);

/* Continuous integrate-and-fire.  Launch 1, one thread per row over steps t = 0 .. len[b] (len[b] + 1 dependent fp32 additions):
 *   comp = 1 - integrate; integrate += alpha_t; fire = integrate >= threshold; if fire: integrate -= 1; cur_t = fire ? comp : alpha_t
 * recording cur f32 [B][ld_alpha], and per fire k < L_cap its step pos int [B][L_cap] and remainder rem f32 [B][L_cap] = alpha_t -
 * cur_t; count int [B] = ALL fires of the row.  Launch 2, per (row, token k, channel): frame = rem_{k-1} h[pos_{k-1}] (0 for
 * k = 0), then frame += cur_t h_t for t = pos_{k-1} + 1 .. pos_k in time order, product and sum rounded separately: the bits of
 * the sequential loop for equal alpha and h.  h f32 [B * T][ldh >= D] is read only at t < len[b]; the step t = len[b] has h = 0.
 * out f32 [B][L_cap][ldo >= D]: token k < min(count[b], L_cap, n_limit[b]) (n_limit DEVICE int [B] or NULL), ZERO beyond. */
F5E_API int f5e_cif_fire_f32(f5e_stream st, const float* alpha, int ld_alpha, const float* h, int ldh, const int* len,
                     const int* n_limit, float* cur, int* pos, float* rem, int* count, float* out, int ldo, int B, int T, int D,
                     int L_cap, float threshold);

/* The pick of the non-autoregressive decoder.  Launch 1, one wave per token row r = b L + k with k < n[b], ONE pass over
 * logits[r][0 .. V) (row stride ld; logits or log-probabilities alike): arg[r] = argmax (lowest index on ties) and logp[r] = its
 * log-softmax value; rows k >= n[b] get -1 and 0.  Launch 2, one wave per utterance: ids int [B][L] = the arg of tokens k < n[b]
 * other than sos, eos and blank, in order, padded with `pad`; len_out int [B] their count; score f32 [B] = sum_{k < n[b]} logp.
 * n DEVICE int [B] clamped to [0, L] (NULL: L). */
F5E_API int f5e_nar_pick(f5e_stream st, const float* logits, long long ld, const int* n, int* arg, float* logp, int* ids,
                 int* len_out, float* score, int B, int L, int V, int sos, int eos, int blank, int pad);

/* ---------------------------------------------------------------- Qwen2 chat model (csrc/llm.hip) -------------- */
/* What a Qwen2-style decoder-only language model needs around f5e_gemm_f32_w16 (prefill) and f5e_gemm_f32_w16_skinny (decode):
 * DESIGN 4s.  fp32 throughout.  No allocation, no synchronisation, no floating-point atomics, no workgroup waits for another;
 * every reduction runs in a fixed order, so a launch is bit-reproducible, capturable, and a row's result does not depend on
 * how many rows the call has.  What changes per token is read on the device: ids, `last`, and the step record `rec` of the
 * Whisper step (DEVICE i32 [8], 16-byte aligned: rec[0] = p, rec[2] / rec[3] = the seed's low / high word). */

/* y[m][:] = (x[m][:] * rsqrt(mean(x[m][:]^2) + eps)) * w, the products in that order (Qwen2RMSNorm in fp32).  x f32 [M][ldx],
 * w f32 [D], out f32 [M][ldo]; out may be x.  One wave per row.  D % 4 == 0, strides multiples of 4 floats, 16-byte aligned
 * (else F5E_ERR_BAD_SHAPE); D <= 8192 (else F5E_ERR_UNSUPPORTED). */
F5E_API int f5e_rmsnorm_f32(f5e_stream st, const float* x, int ldx, const float* w, float* out, int ldo, int M, int D, float eps);
/* out[m][i] = silu(gu[m][i]) * gu[m][I + i], silu(x) = x / (1 + expf(-x)) with the accurate expf.  gu f32 [M][ld >= 2 I] (the
 * fused gate | up projection), out f32 [M][ldo >= I]; I % 4 == 0, strides multiples of 4 floats, 16-byte aligned. */
F5E_API int f5e_swiglu_f32(f5e_stream st, const float* gu, int ld, float* out, int ldo, int M, int I);
/* out[i][:] = emb[ids[i]][:] for i < n, widened exactly (csrc/w_load.h).  ids DEVICE i32 [n], clamped to the table; emb
 * [table_rows][D] f32 (16-byte aligned) or fp16 / bf16 (wtype = F5E_W_*, 8-byte aligned); out f32 [n][D], D % 4 == 0.  The ids
 * are read on the device, so the decode step's form is this call with ids = last and n = R: it needs no position. */
F5E_API int f5e_llm_embed_f32(f5e_stream st, const int* ids, const float* emb, float* out, int n, int D, int table_rows);
F5E_API int f5e_llm_embed_w16(f5e_stream st, const int* ids, const void* emb, int wtype, float* out, int n, int D, int table_rows);
/* Attention with rotary positions and grouped heads.  qkv f32 [rows][ld_qkv >= (H + 2 Hkv) dk] packed q | k | v; kc / vc the
 * layer's f32 caches, element (r, j, c) at r*row_stride + j*pos_stride + c, c < Hkv*dk; begin DEVICE i32 [R] or NULL: the
 * row's left padding; cos / sin f32 [max_pos][dk/2], max_pos >= the cached positions.  Query head h uses key/value head
 * h / (H / Hkv).  Position j of row r is rotated at pos = max(j - begin[r], 0):
 *   x'[d] = x[d] cos[pos][d] - x[d + dk/2] sin[pos][d] (d < dk/2), x[d] cos[pos][d - dk/2] + x[d - dk/2] sin[pos][d - dk/2]
 * (otherwise); two products and one addition per element.  K is filed in the cache rotated, V bit for bit.
 * Limits: dk in {32, 64, 128}, 1 <= H / Hkv <= 8, at most 4096 cached positions (else F5E_ERR_UNSUPPORTED); strides multiples
 * of 4 floats, pointers 16-byte aligned, R, H <= 65535 (else F5E_ERR_BAD_SHAPE).  A row's output equals its R = 1 call's.
 *
 * f5e_gqa_rope_append_f32: the U new positions p0 .. p0+U-1 (row r*U + u of qkv / out) behind p0 cached ones, with the masking,
 * containment and read / write rules of f5e_attn_append_f32 (begin clamped to [0, p0 + U]; cached keys from the caches, new keys
 * from qkv under the causal mask; only slots [r][p0 .. p0+U-1] are written and only slots below p0 read; a query below begin[r]
 * gives exact zeros) on its wave tile.  p0 = 0 is the prefill, p0 > 0 the next turn of a conversation.
 *
 * f5e_gqa_rope_decode_dev_f32: one position p = clamp(rec[0], 0, P - 1), qkv / out f32 [R][..].  Grid (Hkv, R), independent of
 * p: one workgroup serves the H / Hkv query heads of its group and reads every cached element once for all of them; keys are
 * split over the waves of its 512 threads, maxima, sums and partial outputs merged through LDS in a fixed order.  begin
 * clamped to [0, p].
 * Slot [r][p] receives the step's key (rotated) and value; no other slot is written. */
F5E_API int f5e_gqa_rope_append_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                            int pos_stride, const int* begin, const float* cos, const float* sin, int max_pos, float* out,
                            int ldo, int R, int U, int Umax, int H, int Hkv, int dk, int p0, float scale);
F5E_API int f5e_gqa_rope_decode_dev_f32(f5e_stream st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                                int pos_stride, const int* begin, const float* cos, const float* sin, int max_pos, float* out,
                                int ldo, int R, int P, int H, int Hkv, int dk, const int* rec, float scale);
/* The pick of transformers' sampling call, one workgroup per row, the logits [R][ld >= V] read once, at
 * p = clamp(rec[0], 0, n_tok - 2) (n_tok = the columns of a token row, ld_tok its stride):
 *   1. repetition penalty: every class that occurs in tokens[r][begin[r] .. p] gets x < 0 ? x * penalty : x / penalty, once;
 *   2. do_sample = 0: the lowest index among the maxima;
 *   3. do_sample = 1: x / temperature; exactly the top_k largest survive (the lower id first on equal values:
 *      TopKLogitsWarper keeps every class tied with the k-th); softmax over them; in ascending order of probability a survivor
 *      is dropped while the cumulative sum up to and including it is <= 1 - top_p, never the largest (TopPLogitsWarper);
 *      the first survivor, in descending order, whose sequential fp32 cumulative sum reaches u * total is drawn,
 *      u = ((w >> 8) + 0.5) 2^-24 from word 0 of Philox4x32-10(counter = (0, p, serial[r], row_key[r]), key = the seed);
 *   4. tokens[r][p + 1] and last[r] = the pick; done[r] 0 -> 1 on any of the n_eos <= 4 ids of the HOST array eos; a row that
 *      is done writes `pad`; then one workgroup writes *alive = rows not done and rec[0] += 1.
 * keep_id i32 [R][64], keep_p f32 [R][64], keep_n i32 [R] (each may be NULL): the survivors in descending order, their
 * renormalised probabilities and their count (greedy: the pick, 1 and 1; a done row: count 0).  Nothing else is written.
 * penalty >= 1, temperature > 0, 0 < top_p <= 1 (else F5E_ERR_BAD_SHAPE); 1 <= top_k <= min(64, V), 2 <= V <= 262144 (else
 * F5E_ERR_UNSUPPORTED). */
F5E_API int f5e_llm_pick_dev(f5e_stream st, const float* logits, long long ld, int* tokens, int ld_tok, int n_tok, const int* begin,
                     int* last, int* done, int* alive, int R, int V, int* rec, int do_sample, float penalty, float temperature,
                     int top_k, float top_p, const int* eos, int n_eos, int pad, const int* row_key, const int* serial,
                     int* keep_id, float* keep_p, int* keep_n);

/* ---------------------------------------------------------------- hipGraph capture --------------------------- */
F5E_API int f5e_graph_begin(f5e_stream st);
F5E_API int f5e_graph_end(f5e_stream st, void** graph_exec_out);
F5E_API int f5e_graph_launch(void* graph_exec, f5e_stream st);
F5E_API int f5e_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* F5E_ABI_H_ */

// Parakeet, text side (gfx950): TDT, RNNT and CTC greedy decoding on the device.  Restates the prediction network and joint of
// mlx_audio/stt/models/parakeet/rnnt.py:37-157 and the greedy loops of parakeet.py:307-391 (TDT), :411-488 (RNNT) and the head of ctc.py:33-34;
// DESIGN 8t.  All rows of a batch (<= 16) advance in lock step, every row's state lives on the device, the host reads no token inside the loop.
//
// The invariant of every kernel here: a row's bits depend on that row's inputs alone.  Reduction orders are functions of K alone, partial results are
// merged in index order, the only atomic is the integer count of live rows.
//
// Both matrix kernels put the WEIGHTS on the 16-row A side of v_mfma_f32_16x16x32_bf16 and the <= 16 batch rows on the B side, so that lane (lr, g)
// ends with D[weight row 4 g + r][batch row lr], r = 0 .. 3: four consecutive weight rows of ONE batch row in one lane.
//
// ---- lstm_cell_rows: one LSTM layer, one time step --------------------------------------------------------------------------------------------
//   W = [Wx | Wh] along K, its 4 H gate rows (MLX order i, f, g, o) permuted so that row 16 tile + 4 u + gate is gate `gate` of hidden unit
//   4 tile + u, and stored in fragment order [H / 4][K / 32][64 lanes][8]: a wave's load of a k-step is one contiguous KiB.  With the layout above
//   a lane's four accumulators ARE i, f, g, o of unit 4 tile + g for batch row lr: the cell c' = s(f) c + s(i) tanh(g), h' = s(o) tanh(c') runs in
//   that lane in fp32, and the 4 H pre-activations never leave the workgroup.  One workgroup = one tile, 4 waves; wave w takes the k-steps
//   [w per, (w + 1) per), per = ceil(K / 32 / 4), requests up to LSTM_FLIGHT of its weight fragments before the first MFMA, and the four partial
//   tiles are added through LDS in wave order.  The B fragment of batch row lr is [x | h] rounded to bf16: x is the row of the bf16 embedding
//   table of the row's last token (zeros for the blank), or an fp32 row; h is the COMMITTED copy h[idx[lr]], and the results go to the other copy.
//   Rows whose mask is clear are neither computed (zero fragments) nor written; with no row flagged a workgroup returns before its first load.
//
// ---- joint_argmax: logits = act(encp[b][t[b]] + predp[b]) Wout^T + bias, and their arg-maxima -------------------------------------------------
//   A = the dense row-major bf16 [C][Hj] matrix (16 bytes of a row are a fragment), one workgroup per 16 classes, 4 waves over the k-steps as
//   above.  The B fragment is made on the fly: the add in fp32, the activation, one rounding to bf16.  The CTC form of the same kernel takes plain
//   feature rows (fp32 or bf16) in tiles of 16 through blockIdx.y.  After the wave-order sum and the bias, a lane holds four consecutive classes
//   of its batch row; it keeps (max, lowest index) for the token range [0, V1) and the duration range [V1, C), the four lane groups are combined
//   by xor-butterflies, and the workgroup writes one partial per row and range.  The boundary may fall inside a tile.  argmax_merge / decide
//   walk the tiles in index order and replace on strictly greater, so the lowest index wins among equals.
//
// ---- decide: one workgroup, thread b = row b ----------------------------------------------------------------------------------------------
//   merges the partials, applies the TDT or RNNT rule as the reference writes it, appends (token, frame, duration index), moves t, flips the commit
//   index, sets the "needs prediction" flag and takes the row out of the live count when it ends, fills its buffer or reaches its step cap.
#include "kk_host.h"
#include "../../include/kokoro_hip.h"

#include <limits.h>
#include <math.h>

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PT_WAVES = 4, LSTM_FLIGHT = 10, JOINT_FLIGHT = 8;
enum { ST_T, ST_LEN, ST_LAST, ST_IDX, ST_NEED, ST_NEWSYM, ST_COUNT, ST_STEPS, ST_DONE, ST_LIVE, ST_FIELDS };  // int state, [field][16]

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ bf16x8 round8(const float4& a, const float4& b) {
  return bf16x8{(bf16_t)a.x, (bf16_t)a.y, (bf16_t)a.z, (bf16_t)a.w, (bf16_t)b.x, (bf16_t)b.y, (bf16_t)b.z, (bf16_t)b.w};
}

// ------------------------------------------------------------------------------------------------------------------------------ LSTM cell
struct LstmArgs {
  const bf16_t* w;      // fragment pack [H / 4][K / 32][64][8]
  const float* bias;    // [4 H], permuted like W's rows
  const bf16_t* embed;  // [n_embed][in], or null: x is read
  const int* token;     // [M] (embed form)
  int blank, n_embed;
  const float* x;       // fp32 rows at pitch ldx; xcs != 0: copy 1 - idx[b] of a two-copy buffer (the proposed state of the layer below)
  long long ldx, xcs;
  float *h, *c;         // [2][rows][H], copies cs elements apart
  long long cs;
  float* h_out;         // also h' as dense rows [M][H], or null
  const int *idx, *mask;
  int M, in, H;
};

__global__ __launch_bounds__(64 * PT_WAVES) void lstm_cell_rows_kernel(LstmArgs a) {
  __shared__ f32x4 red[PT_WAVES][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4, tile = blockIdx.x;
  const bool on = lr < a.M && a.mask[lr] != 0;
  if (__ballot(on) == 0) return;  // (every wave sees the same 16 flags: uniform over the workgroup)
  const int KS = (a.in + a.H) >> 5, per = (KS + PT_WAVES - 1) / PT_WAVES;
  const int lo = wave * per, hi = lo + per < KS ? lo + per : KS;
  const int ci = on ? (a.idx[lr] & 1) : 0;
  const bf16_t* xe = nullptr;  // the embedding row, or null (blank: zeros)
  const float* xf = nullptr;
  if (on) {
    if (a.embed) {
      const int tok = a.token[lr];
      if (tok != a.blank && tok >= 0 && tok < a.n_embed) xe = a.embed + (long long)tok * a.in;
    } else {
      xf = a.x + (a.xcs ? (long long)(1 - ci) * a.xcs : 0) + (long long)lr * a.ldx;
    }
  }
  const float* hp = a.h + (long long)ci * a.cs + (long long)lr * a.H;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  auto frag = [&](int ks) __attribute__((always_inline)) -> bf16x8 {
    const int k = 32 * ks + 8 * g;
    if (!on) return zero;
    if (k < a.in) {
      if (a.embed) return xe ? *(const bf16x8*)(xe + k) : zero;
      return round8(*(const float4*)(xf + k), *(const float4*)(xf + k + 4));
    }
    return round8(*(const float4*)(hp + k - a.in), *(const float4*)(hp + k - a.in + 4));
  };
  const bf16x8* wp = (const bf16x8*)a.w + (long long)tile * KS * 64 + lane;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = lo; k0 < hi; k0 += LSTM_FLIGHT) {
    bf16x8 wf[LSTM_FLIGHT];
#pragma unroll
    for (int j = 0; j < LSTM_FLIGHT; ++j) wf[j] = k0 + j < hi ? wp[(long long)(k0 + j) * 64] : zero;
#pragma unroll
    for (int j = 0; j < LSTM_FLIGHT; ++j)
      if (k0 + j < hi) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], frag(k0 + j), acc, 0, 0, 0);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0 || !on) return;
  f32x4 v = red[0][lane];
#pragma unroll
  for (int w = 1; w < PT_WAVES; ++w) v += red[w][lane];
  const int u = 4 * tile + g;  // this lane's hidden unit; v = its gates i, f, g, o
  const f32x4 b = *(const f32x4*)(a.bias + 16 * tile + 4 * g);
  const float gi = sigmoid_f32(v[0] + b[0]), gf = sigmoid_f32(v[1] + b[1]), gg = tanhf(v[2] + b[2]), go = sigmoid_f32(v[3] + b[3]);
  const long long src = (long long)ci * a.cs + (long long)lr * a.H + u, dst = (long long)(1 - ci) * a.cs + (long long)lr * a.H + u;
  const float cn = gf * a.c[src] + gi * gg, hn = go * tanhf(cn);
  a.c[dst] = cn;
  a.h[dst] = hn;
  if (a.h_out) a.h_out[(long long)lr * a.H + u] = hn;
}

// ------------------------------------------------------------------------------------------------------------------------------ joint
struct JointArgs {
  const bf16_t* w;    // [C][K] dense
  const float* bias;  // [C]
  int C, K, V1;       // token range [0, V1), duration range [V1, C)
  const float* encp;  // joint form: [M][T_rows][K] fp32, row b at b * ebs
  long long ebs;
  int T_rows;
  const int* t;
  const float* predp;  // [M][K]
  int act;             // 0 relu, 1 sigmoid, 2 tanh
  const void* feat;    // CTC form: rows x K at pitch ldf, fp32 or bf16
  int feat_bf16;
  long long ldf;
  int rows;            // rows in all (joint form: M)
  float* logits;       // [rows][ldl] or null
  long long ldl;
  float* pmax;         // [row tile][class tile][2][16]
  int* pidx;
};

__device__ __forceinline__ void better(float& m, int& i, float om, int oi) {
  if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}

template <bool CTC>
__global__ __launch_bounds__(64 * PT_WAVES) void joint_argmax_kernel(JointArgs a) {
  __shared__ f32x4 red[PT_WAVES][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4, tile = blockIdx.x, rt = blockIdx.y;
  const int row = 16 * rt + lr;
  const bool on = row < a.rows;
  const int KS = a.K >> 5, per = (KS + PT_WAVES - 1) / PT_WAVES;
  const int lo = wave * per, hi = lo + per < KS ? lo + per : KS;
  const int cr = 16 * tile + lr < a.C ? 16 * tile + lr : a.C - 1;  // the tail's classes read the last row; they are not stored
  const bf16_t* wp = a.w + (long long)cr * a.K + 8 * g;
  const float *ep = nullptr, *pp = nullptr;
  const char* fp = nullptr;
  if (on) {
    if constexpr (CTC) {
      fp = (const char*)a.feat + (long long)row * a.ldf * (a.feat_bf16 ? 2 : 4);
    } else {
      int tt = a.t[row];
      tt = tt < 0 ? 0 : (tt >= a.T_rows ? a.T_rows - 1 : tt);  // an ended row stands past its last frame: its result is not used
      ep = a.encp + (long long)row * a.ebs + (long long)tt * a.K;
      pp = a.predp + (long long)row * a.K;
    }
  }
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  auto act1 = [&](float v) __attribute__((always_inline)) { return a.act == 0 ? fmaxf(v, 0.f) : (a.act == 1 ? sigmoid_f32(v) : tanhf(v)); };
  auto frag = [&](int ks) __attribute__((always_inline)) -> bf16x8 {
    const int k = 32 * ks + 8 * g;
    if (!on) return zero;
    if constexpr (CTC) {
      if (a.feat_bf16) return *(const bf16x8*)(fp + 2 * k);
      return round8(*(const float4*)(fp + 4 * k), *(const float4*)(fp + 4 * k + 16));
    } else {
      const float4 e0 = *(const float4*)(ep + k), e1 = *(const float4*)(ep + k + 4), p0 = *(const float4*)(pp + k), p1 = *(const float4*)(pp + k + 4);
      return round8(float4{act1(e0.x + p0.x), act1(e0.y + p0.y), act1(e0.z + p0.z), act1(e0.w + p0.w)},
                    float4{act1(e1.x + p1.x), act1(e1.y + p1.y), act1(e1.z + p1.z), act1(e1.w + p1.w)});
    }
  };
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = lo; k0 < hi; k0 += JOINT_FLIGHT) {
    bf16x8 wf[JOINT_FLIGHT];
#pragma unroll
    for (int j = 0; j < JOINT_FLIGHT; ++j) wf[j] = k0 + j < hi ? *(const bf16x8*)(wp + 32 * (k0 + j)) : zero;
#pragma unroll
    for (int j = 0; j < JOINT_FLIGHT; ++j)
      if (k0 + j < hi) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], frag(k0 + j), acc, 0, 0, 0);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
  f32x4 v = red[0][lane];
#pragma unroll
  for (int w = 1; w < PT_WAVES; ++w) v += red[w][lane];
  float m0 = -INFINITY, m1 = -INFINITY;
  int i0 = INT_MAX, i1 = INT_MAX;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int cls = 16 * tile + 4 * g + r;
    if (cls >= a.C) continue;
    const float x = v[r] + a.bias[cls];
    if (on && a.logits) a.logits[(long long)row * a.ldl + cls] = x;
    if (cls < a.V1) better(m0, i0, x, cls);
    else better(m1, i1, x, cls - a.V1);
  }
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    better(m0, i0, __shfl_xor(m0, o), __shfl_xor(i0, o));
    better(m1, i1, __shfl_xor(m1, o), __shfl_xor(i1, o));
  }
  if (g == 0) {
    const long long p = (((long long)rt * gridDim.x + tile) * 2) * 16 + lr;
    a.pmax[p] = m0; a.pidx[p] = i0;
    a.pmax[p + 16] = m1; a.pidx[p + 16] = i1;
  }
}

// the class tiles' partials of (row tile rt, row lr, range) in index order: the first of the largest
__device__ __forceinline__ int merge_partials(const float* pmax, const int* pidx, int ntile, int rt, int lr, int range) {
  float best = -INFINITY;
  int idx = -1;
  for (int tile = 0; tile < ntile; ++tile) {
    const long long p = (((long long)rt * ntile + tile) * 2 + range) * 16 + lr;
    const int i = pidx[p];
    if (i != INT_MAX && (idx < 0 || pmax[p] > best)) { best = pmax[p]; idx = i; }
  }
  return idx;
}

__global__ __launch_bounds__(64) void argmax_merge_kernel(const float* pmax, const int* pidx, int ntile, int rows, int* tok, int* dur) {
  const int rt = blockIdx.x, lr = threadIdx.x & 15, range = threadIdx.x >> 4, row = 16 * rt + lr;
  if (range > 1 || row >= rows) return;
  int* dst = range ? dur : tok;
  if (dst) dst[row] = merge_partials(pmax, pidx, ntile, rt, lr, range);
}

// ------------------------------------------------------------------------------------------------------------------------------ decide
struct DecideArgs {
  const float* pmax;
  const int* pidx;
  int ntile, M, V, rule, max_symbols, cap, step_cap;  // rule 0 = tdt, 1 = rnnt; max_symbols < 0: none
  int durations[KK_PARAKEET_MAX_DURATIONS];
  int* st;   // [ST_FIELDS][16]
  int* out;  // [M][cap][3]
};

__global__ __launch_bounds__(64) void decide_kernel(DecideArgs a) {
  const int b = threadIdx.x;
  if (b >= a.M) return;
  int* st = a.st;
  if (st[ST_DONE * 16 + b]) { st[ST_NEED * 16 + b] = 0; return; }
  const int tok = merge_partials(a.pmax, a.pidx, a.ntile, 0, b, 0);
  int t = st[ST_T * 16 + b], ns = st[ST_NEWSYM * 16 + b], count = st[ST_COUNT * 16 + b];
  const int steps = st[ST_STEPS * 16 + b] + 1;
  const bool emit = tok != a.V;
  int di = 0;
  if (a.rule == 0) di = merge_partials(a.pmax, a.pidx, a.ntile, 0, b, 1);
  if (emit) {
    int* o = a.out + ((long long)b * a.cap + count) * 3;  // count < cap: a full row has ended
    o[0] = tok; o[1] = t; o[2] = di;
    ++count;
    st[ST_LAST * 16 + b] = tok;
    st[ST_IDX * 16 + b] ^= 1;  // the proposed state is the committed one from here on
  }
  if (a.rule == 0) {  // parakeet.py:378-386
    const int d = a.durations[di];
    t += d;
    ++ns;
    if (d != 0) ns = 0;
    else if (a.max_symbols >= 0 && a.max_symbols <= ns) { ++t; ns = 0; }
  } else if (emit) {  // :477-480
    ++ns;
    if (a.max_symbols >= 0 && a.max_symbols <= ns) { ++t; ns = 0; }
  } else {  // :482-483
    ++t;
    ns = 0;
  }
  int done = 0;
  if (t >= st[ST_LEN * 16 + b]) done = 1;
  else if (count >= a.cap || steps >= a.step_cap) done = 2;  // truncated
  st[ST_T * 16 + b] = t;
  st[ST_NEWSYM * 16 + b] = ns;
  st[ST_COUNT * 16 + b] = count;
  st[ST_STEPS * 16 + b] = steps;
  st[ST_DONE * 16 + b] = done;
  st[ST_NEED * 16 + b] = emit && !done;
  if (done) atomicSub(&st[ST_LIVE * 16], 1);
}

// ------------------------------------------------------------------------------------------------------------------------------ checks and launches
int check_lstm(const char* who, int M, int in, int H) {
  if (M < 1 || M > KK_PARAKEET_TEXT_MAX_ROWS) return kk_failf("%s: M = %d must be in [1, %d]", who, M, KK_PARAKEET_TEXT_MAX_ROWS);
  if (in < 32 || in % 32 != 0) return kk_failf("%s: the input width %d is not a multiple of 32", who, in);
  if (H < 32 || H % 32 != 0) return kk_failf("%s: H = %d is not a multiple of 32", who, H);
  return 0;
}
int launch_lstm(hipStream_t st, const LstmArgs& a) {
  hipLaunchKernelGGL(lstm_cell_rows_kernel, dim3(a.H / 4), dim3(64 * PT_WAVES), 0, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}
int check_joint(const char* who, int rows, int max_rows, int K, int C, int V1, int act) {
  if (rows < 1 || rows > max_rows) return kk_failf("%s: M = %d must be in [1, %d]", who, rows, max_rows);
  if (K < 32 || K % 32 != 0) return kk_failf("%s: K = %d is not a multiple of 32", who, K);
  if (C < 1 || V1 < 1 || V1 > C || C > (1 << 24)) return kk_failf("%s: need 1 <= V1 <= C", who);
  if (act < 0 || act > 2) return kk_failf("%s: unknown activation %d (0 relu, 1 sigmoid, 2 tanh)", who, act);
  return 0;
}
size_t joint_scratch_bytes(int rows, int C) { return (size_t)((rows + 15) / 16) * ((C + 15) / 16) * 2 * 16 * 8; }
// a.pmax / a.pidx are set here from `scratch`
int launch_joint(hipStream_t st, JointArgs a, bool ctc, void* scratch) {
  const int rts = (a.rows + 15) / 16, ntile = (a.C + 15) / 16;
  a.pmax = (float*)scratch;
  a.pidx = (int*)scratch + (size_t)rts * ntile * 32;
  if (ctc) hipLaunchKernelGGL(joint_argmax_kernel<true>, dim3(ntile, rts), dim3(64 * PT_WAVES), 0, st, a);
  else hipLaunchKernelGGL(joint_argmax_kernel<false>, dim3(ntile, rts), dim3(64 * PT_WAVES), 0, st, a);
  KK_CHECK_LAUNCH();
  return 0;
}
int launch_merge(hipStream_t st, void* scratch, int rows, int C, int* tok, int* dur) {
  const int rts = (rows + 15) / 16, ntile = (C + 15) / 16;
  hipLaunchKernelGGL(argmax_merge_kernel, dim3(rts), dim3(64), 0, st, (const float*)scratch, (const int*)scratch + (size_t)rts * ntile * 32, ntile, rows, tok, dur);
  KK_CHECK_LAUNCH();
  return 0;
}

// [Wx | Wh] and the bias in the kernel's order (host)
void pack_lstm(const float* wx, const float* wh, const float* bias, int in, int H, uint16_t* w_out, float* bias_out) {
  const int K = in + H, KS = K / 32;
  for (int tile = 0; tile < H / 4; ++tile)
    for (int lr = 0; lr < 16; ++lr) {
      const long long src = (long long)(lr & 3) * H + 4 * tile + (lr >> 2);  // gate lr & 3 of unit 4 tile + (lr >> 2)
      bias_out[16 * tile + lr] = bias ? bias[src] : 0.f;
      for (int k = 0; k < K; ++k) {
        const float v = k < in ? wx[src * in + k] : wh[src * H + (k - in)];
        w_out[(((long long)tile * KS + (k >> 5)) * 64 + ((k & 31) >> 3) * 16 + lr) * 8 + (k & 7)] = f32_to_bf16_rne(v);
      }
    }
}
}  // namespace

// ============================================================================================================================ raw entries
extern "C" size_t kk_op_lstm_pack_elems(int in, int H) { return in < 1 || H < 1 ? 0 : (size_t)4 * H * ((size_t)in + H); }

extern "C" int kk_op_lstm_pack(const float* wx, const float* wh, const float* bias, int in, int H, void* w_out, float* bias_out) {
  const char* who = "kk_op_lstm_pack";
  if (!wx || !wh || !w_out || !bias_out) return kk_failf("%s: null argument", who);
  KK_TRY(check_lstm(who, 1, in, H));
  pack_lstm(wx, wh, bias, in, H, (uint16_t*)w_out, bias_out);
  return 0;
}

extern "C" int kk_op_lstm_cell_rows(void* stream, int M, int in, int H, const void* w_packed, const float* bias_packed, const void* embed, int n_embed,
                                    const int32_t* token, int blank, const float* x, long long ldx, float* h, float* c, long long copy_stride,
                                    const int32_t* idx, const int32_t* mask) {
  const char* who = "kk_op_lstm_cell_rows";
  KK_TRY(check_lstm(who, M, in, H));
  if (!w_packed || !bias_packed || !h || !c || !idx || !mask || (embed ? !token : !x)) return kk_failf("%s: null argument", who);
  if (embed ? n_embed < 1 : ldx < in || ldx % 4 != 0) return kk_failf("%s: need n_embed >= 1, or ldx >= in and a multiple of 4", who);
  if (copy_stride < (long long)M * H) return kk_failf("%s: copy_stride is smaller than M H", who);
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)bias_packed & 15) || ((uintptr_t)embed & 15) || ((uintptr_t)x & 15) || ((uintptr_t)h & 15) || copy_stride % 4 != 0)
    return kk_failf("%s: w, bias, embed, x and h must be 16-byte aligned and copy_stride a multiple of 4", who);
  LstmArgs a{(const bf16_t*)w_packed, bias_packed, (const bf16_t*)embed, token, blank, n_embed, x, ldx, 0, h, c, copy_stride, nullptr, idx, mask, M, in, H};
  return launch_lstm((hipStream_t)stream, a);
}

extern "C" size_t kk_op_joint_argmax_scratch_bytes(int rows, int C) { return rows < 1 || C < 1 ? 0 : joint_scratch_bytes(rows, C); }

extern "C" int kk_op_joint_argmax(void* stream, int M, int Hj, int C, int V1, int act, const void* w, const float* bias, const float* encp, int T_rows,
                                  const int32_t* t, const float* predp, float* logits, void* scratch, size_t scratch_bytes, int32_t* tok, int32_t* dur) {
  const char* who = "kk_op_joint_argmax";
  KK_TRY(check_joint(who, M, KK_PARAKEET_TEXT_MAX_ROWS, Hj, C, V1, act));
  if (!w || !bias || !encp || !t || !predp || !scratch || !tok || T_rows < 1) return kk_failf("%s: null argument", who);
  if (scratch_bytes < joint_scratch_bytes(M, C)) return kk_failf("%s: scratch too small", who);
  if (((uintptr_t)w & 15) || ((uintptr_t)encp & 15) || ((uintptr_t)predp & 15) || ((uintptr_t)scratch & 15)) return kk_failf("%s: w, encp, predp and scratch must be 16-byte aligned", who);
  JointArgs a{(const bf16_t*)w, bias, C, Hj, V1, encp, (long long)T_rows * Hj, T_rows, t, predp, act, nullptr, 0, 0, M, logits, C, nullptr, nullptr};
  KK_TRY(launch_joint((hipStream_t)stream, a, false, scratch));
  return launch_merge((hipStream_t)stream, scratch, M, C, tok, dur);
}

extern "C" int kk_op_ctc_argmax(void* stream, int rows, int K, int C, const void* w, const float* bias, const void* feat, int feat_dtype, long long ldf,
                                float* logits, void* scratch, size_t scratch_bytes, int32_t* ids) {
  const char* who = "kk_op_ctc_argmax";
  KK_TRY(check_joint(who, rows, 1 << 20, K, C, C, 0));
  if (!w || !bias || !feat || !scratch || !ids) return kk_failf("%s: null argument", who);
  if (feat_dtype != KK_F32 && feat_dtype != KK_BF16) return kk_failf("%s: features must be fp32 or bf16", who);
  if (ldf < K || ldf % 8 != 0) return kk_failf("%s: ldf must be >= K and a multiple of 8", who);
  if (scratch_bytes < joint_scratch_bytes(rows, C)) return kk_failf("%s: scratch too small", who);
  if (((uintptr_t)w & 15) || ((uintptr_t)feat & 15) || ((uintptr_t)scratch & 15)) return kk_failf("%s: w, feat and scratch must be 16-byte aligned", who);
  JointArgs a{(const bf16_t*)w, bias, C, K, C, nullptr, 0, 0, nullptr, nullptr, 0, feat, feat_dtype == KK_BF16, ldf, rows, logits, C, nullptr, nullptr};
  KK_TRY(launch_joint((hipStream_t)stream, a, true, scratch));
  return launch_merge((hipStream_t)stream, scratch, rows, C, ids, nullptr);
}

// ============================================================================================================================ the handle
struct kk_parakeet_text {
  kk_parakeet_text_config cfg;
  std::map<std::string, HostTensor> host;
  bool finalized = false;
  bf16_t* wdev = nullptr;
  float* fdev = nullptr;
  int C = 0, n_embed = 0, enc_kp = 0, enc_np = 0;  // classes; embedding rows; joint.enc padded to the MFMA conv kernel's [enc_np][enc_kp]
  size_t embed = 0, enc_w = 0, enc_b = 0, pred_w = 0, pred_b = 0, out_w = 0, out_b = 0;
  std::vector<size_t> lstm_w, lstm_b;
  // the running batch (begin): pointers into the caller's state buffer
  int B = 0, T = 0, cap = 0, step_cap = 0;
  int *st = nullptr, *out = nullptr;
  float *h = nullptr, *c = nullptr, *htop = nullptr, *predp = nullptr, *encp = nullptr;
  bf16_t* featb = nullptr;
  void* scratch = nullptr;
};

extern "C" int kk_parakeet_text_create(const kk_parakeet_text_config* c, kk_parakeet_text** out) {
  const char* who = "kk_parakeet_text_create";
  if (!c || !out) return kk_failf("%s: null argument", who);
  if (c->kind < KK_PARAKEET_TDT || c->kind > KK_PARAKEET_CTC) return kk_failf("%s: kind must be 0 (tdt), 1 (rnnt) or 2 (ctc)", who);
  if (c->vocab < 1 || c->vocab > (1 << 24)) return kk_failf("%s: bad vocab", who);
  if (c->encoder_hidden < 64 || c->encoder_hidden % 64 != 0) return kk_failf("%s: encoder_hidden = %d is not a multiple of 64", who, c->encoder_hidden);
  int nd = 0;
  if (c->kind != KK_PARAKEET_CTC) {
    if (c->pred_hidden < 32 || c->pred_hidden % 32 != 0) return kk_failf("%s: pred_hidden = %d is not a multiple of 32", who, c->pred_hidden);
    if (c->joint_hidden < 32 || c->joint_hidden % 32 != 0) return kk_failf("%s: joint_hidden = %d is not a multiple of 32", who, c->joint_hidden);
    if (c->pred_layers < 1 || c->pred_layers > 8) return kk_failf("%s: pred_layers must be in [1, 8]", who);
    if (c->activation < 0 || c->activation > 2) return kk_failf("%s: unknown activation %d (0 relu, 1 sigmoid, 2 tanh)", who, c->activation);
    if (c->kind == KK_PARAKEET_TDT) {
      nd = c->n_durations;
      if (nd < 1 || nd > KK_PARAKEET_MAX_DURATIONS) return kk_failf("%s: n_durations must be in [1, %d]", who, KK_PARAKEET_MAX_DURATIONS);
      for (int i = 0; i < nd; ++i)
        if (c->durations[i] < 0) return kk_failf("%s: negative duration", who);
    }
  }
  kk_parakeet_text* m = new kk_parakeet_text();
  m->cfg = *c;
  m->C = c->vocab + 1 + nd;
  m->n_embed = c->n_embed > 0 ? c->n_embed : c->vocab + 1;
  *out = m;
  return 0;
}

extern "C" void kk_parakeet_text_destroy(kk_parakeet_text* m) {
  if (!m) return;
  if (m->wdev) (void)hipFree(m->wdev);
  if (m->fdev) (void)hipFree(m->fdev);
  delete m;
}

extern "C" int kk_parakeet_text_load_tensor(kk_parakeet_text* m, const char* name, const int64_t* shape, int ndim, const float* data) {
  return kk_host_load_tensor("kk_parakeet_text_load_tensor", m ? &m->host : nullptr, m && m->finalized, name, shape, ndim, data);
}

// names: embed [n_embed][H]; lstm.<i>.wx [4H][in], .wh [4H][H], .b [4H]; joint.pred.w [Hj][H], .b; joint.enc.w [Hj][De], .b; joint.out.w [C][Hj], .b;
// for CTC only ctc.w [C][De], ctc.b
extern "C" int kk_parakeet_text_finalize(kk_parakeet_text* m, void* stream) {
  const char* who = "kk_parakeet_text_finalize";
  if (!m) return kk_failf("%s: null model", who);
  if (m->finalized) return kk_failf("%s: already finalized", who);
  const kk_parakeet_text_config& c = m->cfg;
  const int H = c.pred_hidden, Hj = c.joint_hidden, De = c.encoder_hidden, C = m->C;
  std::string err;
  std::vector<uint16_t> wpack;
  std::vector<float> fpack;
  auto vec = [&](const std::string& name, int n) -> size_t {
    const size_t off = (fpack.size() + 63) & ~(size_t)63;
    fpack.resize(off + n, 0.f);
    if (const HostTensor* t = kk_host_want(m->host, name, {n}, err)) memcpy(&fpack[off], t->d.data(), (size_t)n * 4);
    return off;
  };
  auto mat = [&](const std::string& name, int N, int K, int Np, int Kp) -> size_t {  // bf16 [Np][Kp], zero padded
    const size_t off = (wpack.size() + 63) & ~(size_t)63;
    wpack.resize(off + (size_t)Np * Kp, 0);
    if (const HostTensor* t = kk_host_want(m->host, name, {N, K}, err))
      for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) wpack[off + (size_t)n * Kp + k] = f32_to_bf16_rne(t->d[(size_t)n * K + k]);
    return off;
  };
  if (c.kind == KK_PARAKEET_CTC) {
    m->out_w = mat("ctc.w", C, De, C, De);
    m->out_b = vec("ctc.b", C);
  } else {
    m->embed = mat("embed", m->n_embed, H, m->n_embed, H);
    for (int i = 0; i < c.pred_layers; ++i) {
      const std::string p = "lstm." + std::to_string(i);
      const size_t woff = (wpack.size() + 63) & ~(size_t)63, boff = (fpack.size() + 63) & ~(size_t)63;
      wpack.resize(woff + (size_t)4 * H * 2 * H, 0);
      fpack.resize(boff + 4 * H, 0.f);
      const HostTensor *wx = kk_host_want(m->host, p + ".wx", {4 * H, H}, err), *wh = kk_host_want(m->host, p + ".wh", {4 * H, H}, err),
                       *b = kk_host_want(m->host, p + ".b", {4 * H}, err);
      if (wx && wh && b) pack_lstm(wx->d.data(), wh->d.data(), b->d.data(), H, H, &wpack[woff], &fpack[boff]);
      m->lstm_w.push_back(woff);
      m->lstm_b.push_back(boff);
    }
    m->pred_w = mat("joint.pred.w", Hj, H, Hj, H);
    m->pred_b = vec("joint.pred.b", Hj);
    m->enc_kp = De;
    m->enc_np = rup(Hj, 128);
    m->enc_w = mat("joint.enc.w", Hj, De, m->enc_np, m->enc_kp);
    const size_t eb = (fpack.size() + 63) & ~(size_t)63;
    fpack.resize(eb + m->enc_np, 0.f);
    if (const HostTensor* t = kk_host_want(m->host, "joint.enc.b", {Hj}, err)) memcpy(&fpack[eb], t->d.data(), (size_t)Hj * 4);
    m->enc_b = eb;
    m->out_w = mat("joint.out.w", C, Hj, C, Hj);
    m->out_b = vec("joint.out.b", C);
  }
  if (!err.empty()) return kk_failf("%s: %s", who, err.c_str());
  hipStream_t st = (hipStream_t)stream;
  if (hipMalloc((void**)&m->wdev, wpack.size() * 2 + 64) != hipSuccess || hipMalloc((void**)&m->fdev, fpack.size() * 4 + 64) != hipSuccess)
    return kk_failf("%s: hipMalloc failed", who);
  if (hipMemcpyAsync(m->wdev, wpack.data(), wpack.size() * 2, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(m->fdev, fpack.data(), fpack.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: upload failed", who);
  m->host.clear();
  m->finalized = true;
  return 0;
}

namespace {
// the caller's state buffer of a batch of B rows x T frames with `cap` tokens per row (TDT / RNNT), or the CTC head's workspace for B x T rows
size_t plan_text(kk_parakeet_text& m, int B, int T, int cap, char* base) {
  Workspace ws;
  ws.base = base;
  ws.cap = (size_t)-1;
  const kk_parakeet_text_config& c = m.cfg;
  const size_t rows = (size_t)B * T;
  if (c.kind == KK_PARAKEET_CTC) {
    m.scratch = ws.raw(joint_scratch_bytes((int)rows, m.C));
    m.out = (int*)ws.raw(rows * 4);
    return ws.used + 256;
  }
  const size_t H = c.pred_hidden, Hj = c.joint_hidden, R = KK_PARAKEET_TEXT_MAX_ROWS;
  m.st = (int*)ws.raw(ST_FIELDS * 16 * 4);
  m.out = (int*)ws.raw((size_t)B * cap * 3 * 4);
  m.h = (float*)ws.raw((size_t)c.pred_layers * 2 * R * H * 4);
  m.c = (float*)ws.raw((size_t)c.pred_layers * 2 * R * H * 4);
  m.htop = (float*)ws.raw(R * H * 4);
  m.predp = (float*)ws.raw(R * Hj * 4);
  m.encp = (float*)ws.raw(rows * Hj * 4);
  m.featb = (bf16_t*)ws.raw(rows * m.enc_kp * 2);
  m.scratch = ws.raw(joint_scratch_bytes((int)R, m.C));
  return ws.used + 256;
}

// LSTM layers 0 .. L - 1 for the rows that need a prediction, then joint.pred of the proposed top state for every row (an unflagged row's is unchanged)
int enqueue_prediction(kk_parakeet_text& m, hipStream_t st) {
  const kk_parakeet_text_config& c = m.cfg;
  const int H = c.pred_hidden, R = KK_PARAKEET_TEXT_MAX_ROWS;
  const long long cs = (long long)R * H;
  for (int l = 0; l < c.pred_layers; ++l) {
    LstmArgs a{m.wdev + m.lstm_w[l], m.fdev + m.lstm_b[l], l == 0 ? m.wdev + m.embed : nullptr, m.st + ST_LAST * 16, c.vocab, m.n_embed,
               l == 0 ? nullptr : m.h + (long long)(l - 1) * 2 * cs, H, l == 0 ? 0 : cs, m.h + (long long)l * 2 * cs, m.c + (long long)l * 2 * cs, cs,
               l + 1 == c.pred_layers ? m.htop : nullptr, m.st + ST_IDX * 16, m.st + ST_NEED * 16, m.B, H, H};
    KK_TRY(launch_lstm(st, a));
  }
  KKLinRows p{m.htop, H, m.wdev + m.pred_w, m.fdev + m.pred_b, nullptr, 0, m.predp, c.joint_hidden, nullptr, 0, nullptr, 0, m.B, c.joint_hidden, H, KK_ACT_NONE};
  return kk_launch_whisper_linear_rows(st, p);
}
}  // namespace

extern "C" size_t kk_parakeet_text_state_bytes(kk_parakeet_text* m, int B, int T, int cap) {
  if (!m || !m->finalized || B < 1 || T < 1 || cap < 1) return 0;
  kk_parakeet_text tmp = *m;  // (plan on a copy: the running batch's pointers stay)
  return plan_text(tmp, B, T, cap, nullptr);
}

// features fp32 [B][T][encoder_hidden] (device), lengths [B] (HOST, each <= T; a row of length 0 ends at once).  TDT / RNNT: joint.enc over all frames, the
// initial prediction (blank input, zero state) and the row state.  Nothing is waited for.
extern "C" int kk_parakeet_text_begin(kk_parakeet_text* m, void* stream, int B, int T, const float* features, const int32_t* lengths, int cap, int step_cap,
                                      void* state, size_t state_bytes) {
  const char* who = "kk_parakeet_text_begin";
  if (!m || !features || !lengths || !state) return kk_failf("%s: null argument", who);
  if (!m->finalized) return kk_failf("%s: model not finalized", who);
  if (m->cfg.kind == KK_PARAKEET_CTC) return kk_failf("%s: a CTC model has no loop: kk_parakeet_text_ctc", who);
  if (B < 1 || B > KK_PARAKEET_TEXT_MAX_ROWS) return kk_failf("%s: B = %d must be in [1, %d]", who, B, KK_PARAKEET_TEXT_MAX_ROWS);
  if (T < 1 || T > (1 << 20) || cap < 1 || cap > (1 << 24) || step_cap < 1) return kk_failf("%s: bad T, cap or step_cap", who);
  if (((uintptr_t)features & 15)) return kk_failf("%s: features must be 16-byte aligned", who);
  for (int b = 0; b < B; ++b)
    if (lengths[b] < 0 || lengths[b] > T) return kk_failf("%s: lengths[%d] = %d is outside [0, T = %d]", who, b, lengths[b], T);
  char* base = (char*)(((uintptr_t)state + 255) & ~(uintptr_t)255);
  if (plan_text(*m, B, T, cap, nullptr) > state_bytes) return kk_failf("%s: state buffer too small", who);
  plan_text(*m, B, T, cap, base);
  m->B = B; m->T = T; m->cap = cap; m->step_cap = step_cap;
  const kk_parakeet_text_config& c = m->cfg;
  const int H = c.pred_hidden, Hj = c.joint_hidden, De = c.encoder_hidden, R = KK_PARAKEET_TEXT_MAX_ROWS;
  hipStream_t st = (hipStream_t)stream;
  int init[ST_FIELDS * 16];
  memset(init, 0, sizeof init);
  int live = 0;
  for (int b = 0; b < 16; ++b) {
    const bool on = b < B && lengths[b] > 0;
    init[ST_LEN * 16 + b] = b < B ? lengths[b] : 0;
    init[ST_LAST * 16 + b] = c.vocab;
    init[ST_NEED * 16 + b] = on;
    init[ST_DONE * 16 + b] = !on;
    live += on;
  }
  init[ST_LIVE * 16] = live;
  if (hipMemcpyAsync(m->st, init, sizeof init, hipMemcpyHostToDevice, st) != hipSuccess) return kk_failf("%s: upload failed", who);
  const size_t hc = (size_t)c.pred_layers * 2 * R * H * 4;
  if (hipMemsetAsync(m->h, 0, hc, st) != hipSuccess || hipMemsetAsync(m->c, 0, hc, st) != hipSuccess || hipMemsetAsync(m->htop, 0, (size_t)R * H * 4, st) != hipSuccess)
    return kk_failf("%s: clearing the state failed", who);
  // encp = joint.enc(features) for all frames, bias folded, on the MFMA conv kernel as a 1-tap conv over B T dense rows
  const int rows = B * T;
  KK_TRY(kk_launch_convert(features, KK_F32, 0, De, m->featb, KK_BF16, 0, m->enc_kp, De, rows, 1, st));
  KKMfmaArgs g;
  memset(&g, 0, sizeof g);
  g.x = m->featb; g.xbs = (long long)rows * m->enc_kp; g.ldx = m->enc_kp; g.w = m->wdev + m->enc_w; g.CinP = m->enc_kp; g.CoutP = m->enc_np; g.Cin = De;
  g.bias = m->fdev + m->enc_b; g.out = m->encp; g.obs = (long long)rows * Hj; g.ldo = Hj; g.Cout = Hj; g.Kw = 1; g.mode = KK_CONV; g.stride = 1; g.dil = 1;
  g.Q = rows; g.Lo_rows = rows; g.lin = KKLen{nullptr, 0, rows}; g.lout = KKLen{nullptr, 0, rows}; g.in_slope = 1.0f; g.scale = 1.0f; g.act = KK_ACT_NONE;
  KK_TRY(kk_launch_conv_mfma(g, 1, KK_F32, st));
  return enqueue_prediction(*m, st);
}

// n decode steps, each joint -> decide -> prediction, with no host sync between them; then (live != null) the count of rows still running is read back,
// which waits for the stream.  Steps after the last row has ended change nothing.
extern "C" int kk_parakeet_text_steps(kk_parakeet_text* m, void* stream, int n, int32_t* live) {
  const char* who = "kk_parakeet_text_steps";
  if (!m || !m->st) return kk_failf("%s: no running batch (kk_parakeet_text_begin)", who);
  if (n < 0) return kk_failf("%s: bad n", who);
  const kk_parakeet_text_config& c = m->cfg;
  hipStream_t st = (hipStream_t)stream;
  const int tdt = c.kind == KK_PARAKEET_TDT;
  JointArgs j{m->wdev + m->out_w, m->fdev + m->out_b, m->C, c.joint_hidden, c.vocab + 1, m->encp, (long long)m->T * c.joint_hidden, m->T, m->st + ST_T * 16,
              m->predp, c.activation, nullptr, 0, 0, m->B, nullptr, 0, nullptr, nullptr};
  DecideArgs d;
  memset(&d, 0, sizeof d);
  d.pmax = (const float*)m->scratch;
  d.ntile = (m->C + 15) / 16;
  d.pidx = (const int*)m->scratch + (size_t)d.ntile * 32;
  d.M = m->B; d.V = c.vocab; d.rule = tdt ? 0 : 1; d.max_symbols = c.max_symbols; d.cap = m->cap; d.step_cap = m->step_cap; d.st = m->st; d.out = m->out;
  for (int i = 0; i < c.n_durations && tdt; ++i) d.durations[i] = c.durations[i];
  for (int s = 0; s < n; ++s) {
    KK_TRY(launch_joint(st, j, false, m->scratch));
    hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(64), 0, st, d);
    KK_CHECK_LAUNCH();
    KK_TRY(enqueue_prediction(*m, st));
  }
  if (live) {
    if (hipMemcpyAsync(live, m->st + ST_LIVE * 16, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return kk_failf("%s: reading the live count failed", who);
  }
  return 0;
}

// counts [B], flags [B] (0 running, 1 ended, 2 truncated), tokens [B][cap][3] = (token, frame, duration index): HOST buffers; waits for the stream
extern "C" int kk_parakeet_text_read(kk_parakeet_text* m, void* stream, int32_t* counts, int32_t* flags, int32_t* tokens) {
  const char* who = "kk_parakeet_text_read";
  if (!m || !m->st) return kk_failf("%s: no running batch (kk_parakeet_text_begin)", who);
  if (!counts || !flags || !tokens) return kk_failf("%s: null argument", who);
  hipStream_t st = (hipStream_t)stream;
  int host[ST_FIELDS * 16];
  if (hipMemcpyAsync(host, m->st, sizeof host, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(tokens, m->out, (size_t)m->B * m->cap * 12, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return kk_failf("%s: download failed", who);
  for (int b = 0; b < m->B; ++b) {
    counts[b] = host[ST_COUNT * 16 + b];
    flags[b] = host[ST_DONE * 16 + b];
  }
  return 0;
}

// the CTC head over `rows` feature rows fp32 [rows][encoder_hidden] (device): ids [rows] (device) = the per-frame arg-maximum of the logits
extern "C" int kk_parakeet_text_ctc(kk_parakeet_text* m, void* stream, int rows, const float* features, int32_t* ids, void* workspace, size_t workspace_bytes) {
  const char* who = "kk_parakeet_text_ctc";
  if (!m || !features || !ids || !workspace) return kk_failf("%s: null argument", who);
  if (!m->finalized || m->cfg.kind != KK_PARAKEET_CTC) return kk_failf("%s: not a finalized CTC model", who);
  if (rows < 1 || rows > (1 << 20)) return kk_failf("%s: bad rows", who);
  void* base = (void*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if (joint_scratch_bytes(rows, m->C) + 256 > workspace_bytes) return kk_failf("%s: workspace too small", who);
  return kk_op_ctc_argmax(stream, rows, m->cfg.encoder_hidden, m->C, m->wdev + m->out_w, m->fdev + m->out_b, features, KK_F32, m->cfg.encoder_hidden, nullptr, base,
                          workspace_bytes - 256, ids);
}

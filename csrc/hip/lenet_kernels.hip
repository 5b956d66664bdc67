// Hand-written gfx950 (CDNA4 / MI355X) kernels for the LeNet-5-class
// training step.  Design notes:
//
// The whole network is ~1 MFLOP per image forward+backward, so on MI355X the
// bound is kernel-launch count and LATENCY (barrier phases, dependent memory
// chains), never FLOPs (SURVEY.md §7 "hard parts").  The reference CUDA
// variant spends 17 launches + 8 memsets per *sample* (SURVEY.md §2.3); here
// one training step of a whole batch is THREE kernels:
//
//   1. k_fwdbwd  — fused forward + backward-data.  One 256-thread workgroup
//      per image; 3 barriers total (thread t owns pool cell t end-to-end:
//      its 16 conv outputs stay in registers from forward into the pool
//      backward); the fc dot products are 16-lane shuffle reductions so no
//      phase has a >32-step dependency chain.  Fuses what the reference ran
//      as 12 separate kernels per sample.
//   2. k_wgrad   — all weight/bias gradients, batch-reduced.  Measured
//      lesson (profiles/, round 1): a chunk-serial design with LDS staging
//      and per-image barriers ran 62 us — latency-chained.  v2 is
//      barrier-free: grid-stride over flattened (image, position) work
//      items, per-thread register accumulators, wave-level __shfl_down
//      reduction, then a handful of hardware fp32 atomics
//      (unsafeAtomicAdd -> global_atomic_add_f32) into the flat gradient
//      bucket.  The fc weight grads use exclusive per-thread ownership of
//      (k,m) pairs — no atomics, plain accumulate-stores.
//   3. k_update  — SGD apply (p += dt*scale*g) fused with gradient zeroing.
//
// On one GPU with nothing between weight-grad and update (no all-reduce,
// no gradient accumulation) the step is TWO kernels: k_wgrad_update is
// k_wgrad with the update as its tail.  Every block arrives once on a
// device ticket and exits; the block that arrives last applies the update
// and zeroes the bucket.  Nothing waits on anything, so there is no grid
// barrier and no spin (a grid barrier costs more than the kernel boundary
// it would replace).
//
// In-block weight grads (PCNN_LENET_WGRAD=inblock) are a different two-kernel
// step for the same case.  k_wgrad_update exists only to redo, from global
// memory, a reduction over values k_fwdbwd already held in registers, and
// its critical path is four or five serial fabric round trips.  Instead:
//
//   1. k_fwdbwd<.., INBLOCK> — as above, but each cell thread also forms its
//      conv (25 + bias) and pool (16 + bias) gradient partials from dz1, a1
//      and the input window in registers; one LDS hop with a fixed-order sum
//      gives the image's 173 conv/pool sums, stored as one row of a
//      [B][176] fp32 slab.  a1, dz1 and dz2 are never stored.
//   2. k_reduce_update — one owner group of 4 lanes per parameter: sums the
//      slab column or the fc outer product over the batch and applies the
//      SGD update.  No atomics, no gradient bucket, no ticket, no fences;
//      results are bit-reproducible.  One branch-free path with every
//      kernel argument and the parameter's state fetched at entry and, up to
//      64 images, every batch load in flight before the first add: one
//      memory round trip where there were three (9.56 against 10.15
//      us/step at bs=64, profiles/r8).  k_fwdbwd_pair was tried the same
//      way, measured slower and left as it was (profiles/r8 section 5).
//
// k_fwdbwd_pair is kernel 1 of that step with two adjacent lanes per pool
// cell and 512-thread blocks (two waves per SIMD), every global load issued
// before the first FMA, pair-reduced weight-grad partials and a wider owner
// split; it is what the step launchers run by default
// (INBLOCK_DEFAULT_VARIANT; 10.05 against 13.80 us/step at bs=64,
// profiles/r6).  k_fwdbwd<.., INBLOCK> stays selectable (variant 0) and
// still serves nothing else differently: TRAIN, EVAL, INFER and wgrad_fuse
// are the template as before.
//
// Every kernel that applies the update (k_update, k_wgrad_update,
// k_reduce_update) has a _mom twin with momentum / Nesterov / weight decay
// and an fp32 velocity bucket, and an _adam twin (Adam with decoupled weight
// decay, fp32 first- and second-moment buckets); the three are
// instantiations of one body with a compile-time OPT selector
// (sgd_update.h), and the plain kernels are what runs when the optimizer is
// the default one.
//
// Numerics: activations AND the large conv preact gradient (dz1) are
// stored bf16/fp16/fp32 (template); ALL arithmetic is fp32 in
// registers/LDS; parameters, gradients, dz and dz2 are fp32.  Loss-metric
// semantics match the reference (sum over samples of ||onehot - y||_2,
// SURVEY.md §0.1 item 3).
//
// Wave width is 64 (CDNA4); block size 256 = 4 waves (k_fwdbwd_pair: 512 =
// 8 waves).

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "../lenet_dims.h"
#include "../pcnn_launch.h"
#include "act_dispatch.h"

namespace pcnn {

using bf16 = __hip_bfloat16;
using fp16 = __half;

#include "sgd_update.h"

__device__ __forceinline__ float sigmoidf_dev(float v) {
  return 1.0f / (1.0f + __expf(-v));
}

template <typename T>
__device__ __forceinline__ float ldf(const T* p) {
  return (float)*p;
}
template <typename T>
__device__ __forceinline__ void stf(T* p, float v) {
  *p = (T)v;
}

// Vectorized loads of 4/8 consecutive activations as fp32.  Callers
// guarantee 8-byte (bf16) / 16-byte (fp32) alignment of p.
__device__ __forceinline__ void ld4f(const bf16* p, float* out) {
  const ushort4 v = *reinterpret_cast<const ushort4*>(p);
  const bf16* e = reinterpret_cast<const bf16*>(&v);
  out[0] = (float)e[0];
  out[1] = (float)e[1];
  out[2] = (float)e[2];
  out[3] = (float)e[3];
}
__device__ __forceinline__ void ld4f(const fp16* p, float* out) {
  const ushort4 v = *reinterpret_cast<const ushort4*>(p);
  const fp16* e = reinterpret_cast<const fp16*>(&v);
  out[0] = (float)e[0];
  out[1] = (float)e[1];
  out[2] = (float)e[2];
  out[3] = (float)e[3];
}
__device__ __forceinline__ void ld4f(const float* p, float* out) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  out[0] = v.x;
  out[1] = v.y;
  out[2] = v.z;
  out[3] = v.w;
}
template <typename T>
__device__ __forceinline__ void ld8f(const T* p, float* out) {
  ld4f(p, out);
  ld4f(p + 4, out + 4);
}

// Vectorized store of 4 consecutive activations (8-byte-aligned bf16 /
// 16-byte-aligned fp32 destination).
__device__ __forceinline__ void st4f(bf16* p, const float* v) {
  bf16 t[4] = {(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
  *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(t);
}
__device__ __forceinline__ void st4f(fp16* p, const float* v) {
  fp16 t[4] = {(fp16)v[0], (fp16)v[1], (fp16)v[2], (fp16)v[3]};
  *reinterpret_cast<uint2*>(p) = *reinterpret_cast<const uint2*>(t);
}
__device__ __forceinline__ void st4f(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// Execution modes for the fused forward kernel.
enum Mode { MODE_TRAIN = 0, MODE_EVAL = 1, MODE_INFER = 2 };

// LDS image of the per-image state.  One single __shared__ object.
// Only the conv/pool parameters (173 floats) are staged; the fc weight
// matrix stays in global memory (L2-resident, read coalesced once per
// phase).
struct FwdLds {
  float a2s[S1_OUT];    // pool activation
  float ys[FC_OUT];     // logits (post-sigmoid)
  float dzs[FC_OUT];    // residual gradient
  float sq[FC_OUT];     // per-class squared error
  // fused weight-grad accumulators (wgrad_fuse mode): conv1 per-channel
  // 5x5 + bias, pool 4x4 + bias
  float gw[C1_CH][C1_K * C1_K + 1];
  float gs1[S1_WSZ + 1];
};

// In-block weight-grad step (slab layout: GSLAB_LD in lenet_dims.h).
// LDS rows of per-thread partials: 26 conv (25 weights + bias sum) then 17
// pool (16 weights + bias sum); odd stride -> conflict-free row writes.
constexpr int IB_CONV = C1_K * C1_K + 1;        // 26
constexpr int IB_LD = IB_CONV + S1_WSZ + 1;     // 43
constexpr int IB_POOL_T0 = 160;  // first pool-owner thread (4-lane aligned)
static_assert(IB_LD % 2 == 1, "odd LDS row stride");
static_assert(C1_CH * IB_CONV <= IB_POOL_T0 &&
                  IB_POOL_T0 + 4 * (S1_WSZ + 1) <= 256 && S1_OUT % 8 == 0 &&
                  S1_PIX % 4 == 0 && OFF_FW <= GSLAB_LD,
              "owner layout");
// One function-local __shared__ array, only present in kernels that call it.
__device__ __forceinline__ float* inblock_rows() {
  __shared__ float rows[S1_OUT * IB_LD];
  return rows;
}

// Phase stamps (diagnostic build only, -DPCNN_LENET_STAMPS; tools/
// phase_stamps.py).  Lane 0 of every wave stores the shader clock at fixed
// points of the two in-block training kernels into a side buffer of its
// own, [blocks][512][ST_N] 64-bit words indexed by thread so the store is
// an ordinary per-lane one.  In the shipped extension the macros are empty
// and no kernel changes.
#ifdef PCNN_LENET_STAMPS
constexpr int ST_N = 16;
__device__ unsigned long long* g_stamps = nullptr;
__device__ int g_stamp_blocks = 0;
#define PCNN_STAMP(i)                                                        \
  do {                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                       \
    if ((threadIdx.x & 63) == 0 && (int)blockIdx.x < g_stamp_blocks)         \
      g_stamps[((size_t)blockIdx.x * 512 + threadIdx.x) * ST_N + (i)] =      \
          __builtin_amdgcn_s_memtime();                                      \
    __builtin_amdgcn_sched_barrier(0);                                       \
  } while (0)
#define PCNN_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define PCNN_STAMP_LDS_DRAIN() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#else
#define PCNN_STAMP(i) ((void)0)
#define PCNN_STAMP_DRAIN() ((void)0)
#define PCNN_STAMP_LDS_DRAIN() ((void)0)
#endif
// Stamp points, the same in k_fwdbwd<INBLOCK> and k_fwdbwd_pair.
enum {
  ST_ENTRY = 0,     // kernel entry
  ST_LOADS = 1,     // input window (pair: and every hoisted load) landed
  ST_CONV = 2,      // conv + pool FMAs and sigmoids done
  ST_BAR1 = 3,      // past barrier 1
  ST_FC = 4,        // fc forward + residual done
  ST_BAR2 = 5,      // past barrier 2 (and the softmax tail)
  ST_BWD = 6,       // fc backward + pool backward done
  ST_WGRAD = 7,     // weight-grad FMAs done
  ST_LDS = 8,       // partials stored to LDS
  ST_BAR3 = 9,      // past barrier 3
  ST_OWNER = 10,    // owner sums done
  ST_END = 11       // last global store drained
};

// Inside the k_fwdbwd template only the INBLOCK instantiations are stamped.
#define IB_STAMP(i)                      \
  do {                                   \
    if constexpr (INBLOCK) PCNN_STAMP(i); \
  } while (0)
#define IB_STAMP_DRAIN()                        \
  do {                                          \
    if constexpr (INBLOCK) PCNN_STAMP_DRAIN();   \
  } while (0)
#define IB_STAMP_LDS_DRAIN()                        \
  do {                                              \
    if constexpr (INBLOCK) PCNN_STAMP_LDS_DRAIN();   \
  } while (0)

// Fused forward + backward-data, one 256-thread workgroup per image.
//
// Dataflow: thread t < 216 OWNS pool cell (o, pr, pc) — it computes the
// cell's 16 conv1 outputs (from the LDS image + staged weights), applies
// sigmoid, keeps them in REGISTERS, computes the pool output, and later
// runs the pool backward for the same 16 positions from those registers.
// That ownership removes the conv->pool and fc-bwd->pool-bwd barriers and
// all cross-thread a1 LDS traffic: the kernel has 3 barriers total
// ({stage} {conv+pool} {fc+residual} {fc-bwd + pool-bwd + loss}).
//
// Every multiply-add of the forward is an explicit fma, in a fixed order.
// Left as `acc += w * x` the compiler chose a different mix of fused and
// unfused operations per instantiation, and y in eval and infer mode
// differed from y in train mode in the last bit.  With the fmas the forward
// is the same arithmetic in every MODE and in k_fwdbwd_pair.
//
// INBLOCK (MODE_TRAIN only) is the first kernel of the in-block weight-grad
// step: the conv and pool weight gradients of this image are formed from
// the registers that already hold dz1, a1 and the input window, reduced
// over the block through LDS in a fixed order, and stored as row b of the
// slab that `grads` points to in this variant (see GSLAB_LD).  a1, dz1 and
// dz2 are then not stored at all, because nothing reads them.
template <typename act_t, int MODE, bool INBLOCK = false>
__global__ __launch_bounds__(256) void k_fwdbwd(
    const act_t* __restrict__ x, const float* __restrict__ params,
    act_t* __restrict__ a1g, act_t* __restrict__ a2g, float* __restrict__ yg,
    float* __restrict__ dzg, float* __restrict__ dz2g,
    act_t* __restrict__ dz1g, const int* __restrict__ labels,
    float* __restrict__ loss_accum, int* __restrict__ correct_accum, int B,
    int pool_mode, int loss_mode, float* __restrict__ grads,
    int wgrad_fuse) {
  __shared__ FwdLds L;
  const int b = blockIdx.x;
  if (b >= B) return;
  const int tid = threadIdx.x;
  IB_STAMP(ST_ENTRY);

  // No staging phase: each thread loads its own 8x8 input window straight
  // from global (overlapping windows hit L1; one 1.5 KB image per block)
  // and the 173 conv/pool parameters broadcast through L1 — the kernel has
  // TWO barriers ({conv+pool} {fc+residual} {bwd}).
  if (MODE == MODE_TRAIN && wgrad_fuse) {
    if (tid < C1_CH * (C1_K * C1_K + 1))
      L.gw[tid / (C1_K * C1_K + 1)][tid % (C1_K * C1_K + 1)] = 0.f;
    else if (tid < C1_CH * (C1_K * C1_K + 1) + S1_WSZ + 1)
      L.gs1[tid - C1_CH * (C1_K * C1_K + 1)] = 0.f;
  }
  const act_t* xb = x + (size_t)b * IN_PIX;

  // ---- phase 1: conv1 + sigmoid + pool + sigmoid (no barrier between) ----
  const int o = tid / S1_PIX;
  const int pq = tid - o * S1_PIX;
  const int pr = pq / S1_W;
  const int pc = pq - pr * S1_W;
  float a1v[S1_K * S1_K];  // this cell's conv activations, kept live to bwd
  float a2v = 0.f;
  float xw[8][8];  // this cell's input window; INBLOCK keeps it live to bwd
  if (tid < S1_OUT) {
    // load the cell's 8x8 input window into registers (2 x 8B loads/row)
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int v4 = 0; v4 < 2; ++v4)
        ld4f(xb + (pr * S1_K + u) * IN_W + pc * S1_K + v4 * 4,
             &xw[u][v4 * 4]);
    const float* w = params + OFF_C1W + o * C1_K * C1_K;
    const float cb = params[OFF_C1B + o];
    IB_STAMP_DRAIN();
    IB_STAMP(ST_LOADS);
    // pool preact: trainable weighted sum (reference) or max
    float pacc = pool_mode == 1 ? -1e30f : params[OFF_S1B];
#pragma unroll
    for (int i = 0; i < S1_K; ++i) {
#pragma unroll
      for (int j = 0; j < S1_K; ++j) {
        float acc = cb;
#pragma unroll
        for (int u = 0; u < C1_K; ++u)
#pragma unroll
          for (int v = 0; v < C1_K; ++v)
            acc = __builtin_fmaf(w[u * C1_K + v], xw[i + u][j + v], acc);
        const float av = sigmoidf_dev(acc);
        a1v[i * S1_K + j] = av;
        if (pool_mode == 1)
          pacc = fmaxf(pacc, av);
        else
          pacc = __builtin_fmaf(params[OFF_S1W + i * S1_K + j], av, pacc);
      }
    }
    if (MODE == MODE_TRAIN && !INBLOCK) {
      // 4-wide activation stores per conv row
#pragma unroll
      for (int i = 0; i < S1_K; ++i)
        st4f(a1g + (size_t)b * C1_OUT + o * C1_PIX +
                 (pr * S1_K + i) * C1_W + pc * S1_K,
             &a1v[i * S1_K]);
    }
    a2v = sigmoidf_dev(pacc);
    L.a2s[tid] = a2v;
    if (MODE == MODE_TRAIN) stf(a2g + (size_t)b * S1_OUT + tid, a2v);
    IB_STAMP(ST_CONV);
  }
  __syncthreads();
  IB_STAMP(ST_BAR1);

  // ---- phase 2: fc (216 -> 10) + sigmoid [+ loss residual] ----
  // 16 lanes per output class, 4-step shuffle tree; the group leader
  // applies bias+sigmoid and computes the residual in-phase.
  if (tid < FC_OUT * 16) {
    const int k = tid >> 4;
    const int l = tid & 15;
    const float* wk = params + OFF_FW + k * FC_IN;
    float p = 0.f;
#pragma unroll
    for (int u = 0; u < (FC_IN + 15) / 16; ++u) {
      const int m = l + u * 16;
      if (m < FC_IN) p = __builtin_fmaf(wk[m], L.a2s[m], p);
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) p += __shfl_down(p, off, 16);
    if (l == 0) {
      const float z = p + params[OFF_FB + k];
      if (loss_mode == 1) {
        L.ys[k] = z;  // raw logit; softmax finished below
      } else {
        const float v = sigmoidf_dev(z);
        L.ys[k] = v;
        if (yg != nullptr) yg[(size_t)b * FC_OUT + k] = v;
        if (MODE == MODE_TRAIN) {
          const float d = (k == labels[b] ? 1.0f : 0.0f) - v;
          L.dzs[k] = d;
          L.sq[k] = d * d;
          dzg[(size_t)b * FC_OUT + k] = d;
        }
      }
    }
    IB_STAMP(ST_FC);
  }
  __syncthreads();
  if (loss_mode == 1) {
    // softmax over the 10 logits + CE residual (dz = onehot - softmax)
    if (tid == 0) {
      float mx = L.ys[0];
#pragma unroll
      for (int k = 1; k < FC_OUT; ++k) mx = fmaxf(mx, L.ys[k]);
      float sum = 0.f;
      float e[FC_OUT];
#pragma unroll
      for (int k = 0; k < FC_OUT; ++k) {
        e[k] = __expf(L.ys[k] - mx);
        sum += e[k];
      }
#pragma unroll
      for (int k = 0; k < FC_OUT; ++k) {
        const float v = e[k] / sum;
        L.ys[k] = v;
        if (yg != nullptr) yg[(size_t)b * FC_OUT + k] = v;
        if (MODE == MODE_TRAIN) {
          const float d = (k == labels[b] ? 1.0f : 0.0f) - v;
          L.dzs[k] = d;
          dzg[(size_t)b * FC_OUT + k] = d;
        }
      }
      if (MODE == MODE_TRAIN)
        L.sq[0] = -__logf(fmaxf(L.ys[labels[b]], 1e-30f));
    }
    __syncthreads();
  }

  if (MODE == MODE_EVAL) {
    // argmax + correct-count (replaces the reference's per-image D2H copy +
    // host argmax, CUDA/main.cu:220)
    if (tid == 0) {
      int best = 0;
      for (int k = 1; k < FC_OUT; ++k)
        if (L.ys[k] > L.ys[best]) best = k;
      if (best == labels[b]) atomicAdd(correct_accum, 1);
    }
    return;
  }
  if (MODE == MODE_INFER) return;

  // ---- phase 3: fc bwd -> pool preact grad -> pool bwd (no barriers) ----
  IB_STAMP(ST_BAR2);
  if (tid < S1_OUT) {
    float da = 0.f;
#pragma unroll
    for (int k = 0; k < FC_OUT; ++k)
      da += params[OFF_FW + k * FC_IN + tid] * L.dzs[k];
    const float d2 = da * a2v * (1.0f - a2v);
    if (!INBLOCK) dz2g[(size_t)b * S1_OUT + tid] = d2;
    // pool backward for this thread's own 16 conv positions (registers):
    // trainable -> d2 * kernel weight everywhere; max -> d2 at the argmax
    int best = 0;
    if (pool_mode == 1) {
      float bv = a1v[0];
#pragma unroll
      for (int t = 1; t < S1_K * S1_K; ++t)
        if (a1v[t] > bv) {
          bv = a1v[t];
          best = t;
        }
    }
    float dz1v[S1_K * S1_K];
#pragma unroll
    for (int i = 0; i < S1_K; ++i) {
#pragma unroll
      for (int j = 0; j < S1_K; ++j) {
        const float av = a1v[i * S1_K + j];
        const float dd =
            pool_mode == 1
                ? (i * S1_K + j == best ? d2 : 0.f)
                : d2 * params[OFF_S1W + i * S1_K + j];
        dz1v[i * S1_K + j] = dd * av * (1.0f - av);
      }
      if (!INBLOCK)
        st4f(dz1g + (size_t)b * C1_OUT + o * C1_PIX +
                 (pr * S1_K + i) * C1_W + pc * S1_K,
             &dz1v[i * S1_K]);
    }
    IB_STAMP(ST_BWD);
    if constexpr (INBLOCK) {
      // conv1 partial of this cell: 16 dz1 x the 8x8 window, all registers
      // (400 FMAs, no loads); pool partial: d2 x the cell's 16 activations.
      // dz1 and a1 enter rounded to the activation dtype, which is what the
      // k_wgrad path reads back from memory, so both paths form the same
      // products and differ only in summation order.  That is a choice made
      // so the two paths stay comparable (same-results table, profiles/r4),
      // not a requirement: the unrounded registers would be more accurate
      // and save 32 conversions per thread.
      float cacc[C1_K * C1_K];
#pragma unroll
      for (int w2 = 0; w2 < C1_K * C1_K; ++w2) cacc[w2] = 0.f;
      float csum = 0.f;
#pragma unroll
      for (int i = 0; i < S1_K; ++i)
#pragma unroll
        for (int j = 0; j < S1_K; ++j) {
          const float d = (float)(act_t)dz1v[i * S1_K + j];
          csum += d;
#pragma unroll
          for (int u = 0; u < C1_K; ++u)
#pragma unroll
            for (int v = 0; v < C1_K; ++v)
              cacc[u * C1_K + v] += d * xw[i + u][j + v];
        }
      IB_STAMP(ST_WGRAD);
      float* row = inblock_rows() + tid * IB_LD;
#pragma unroll
      for (int w2 = 0; w2 < C1_K * C1_K; ++w2) row[w2] = cacc[w2];
      row[C1_K * C1_K] = csum;
      if (pool_mode == 0) {
#pragma unroll
        for (int t = 0; t < S1_WSZ; ++t)
          row[IB_CONV + t] = d2 * (float)(act_t)a1v[t];
        row[IB_CONV + S1_WSZ] = d2;
      }
      IB_STAMP_LDS_DRAIN();
      IB_STAMP(ST_LDS);
    } else if (wgrad_fuse) {
      // conv1 wgrad: this cell's 16 dz1 x its 8x8 input window (from LDS);
      // per-thread register accumulation, LDS-atomic combine per channel,
      // one global atomic per weight per block (in the final phase below).
      float cacc[C1_K * C1_K];
#pragma unroll
      for (int w2 = 0; w2 < C1_K * C1_K; ++w2) cacc[w2] = 0.f;
      float csum = 0.f;
#pragma unroll
      for (int t = 0; t < S1_K * S1_K; ++t) {
        const float d = dz1v[t];
        csum += d;
        const int r = pr * S1_K + t / S1_K;
        const int c = pc * S1_K + (t & 3);
#pragma unroll
        for (int u = 0; u < C1_K; ++u)
#pragma unroll
          for (int v = 0; v < C1_K; ++v)
            cacc[u * C1_K + v] += d * ldf(xb + (r + u) * IN_W + (c + v));
      }
#pragma unroll
      for (int w2 = 0; w2 < C1_K * C1_K; ++w2)
        atomicAdd(&L.gw[o][w2], cacc[w2]);
      atomicAdd(&L.gw[o][C1_K * C1_K], csum);
      if (pool_mode == 0) {
        // pool wgrad: dz2(own cell) x own a1 activations
#pragma unroll
        for (int t = 0; t < S1_K * S1_K; ++t)
          atomicAdd(&L.gs1[t], d2 * a1v[t]);
        atomicAdd(&L.gs1[S1_WSZ], d2);
      }
    }
  } else if (tid == S1_OUT && loss_accum != nullptr) {
    if (loss_mode == 1) {
      unsafeAtomicAdd(loss_accum, L.sq[0]);
    } else {
      float ssum = 0.f;
#pragma unroll
      for (int k = 0; k < FC_OUT; ++k) ssum += L.sq[k];
      unsafeAtomicAdd(loss_accum, sqrtf(ssum));
    }
  }
  if constexpr (INBLOCK) {
    __syncthreads();
    IB_STAMP(ST_BAR3);
    // Owners sum the 216 rows in a fixed order and store this image's slab
    // row with plain stores; the kernel boundary publishes them.
    const float* rows = inblock_rows();
    float* out = grads + (size_t)b * GSLAB_LD;
    if (tid < C1_CH * IB_CONV) {
      // one owner per (channel, 5x5 weight | bias): the channel's 36 cells
      const int o2 = tid / IB_CONV;
      const int w2 = tid - o2 * IB_CONV;
      const float* col = rows + o2 * S1_PIX * IB_LD + w2;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
      for (int c = 0; c < S1_PIX; c += 4) {
        s0 += col[(c + 0) * IB_LD];
        s1 += col[(c + 1) * IB_LD];
        s2 += col[(c + 2) * IB_LD];
        s3 += col[(c + 3) * IB_LD];
      }
      const float v = ((s0 + s1) + (s2 + s3)) * (1.0f / (float)C1_PIX);
      IB_STAMP(ST_OWNER);
      out[w2 < C1_K * C1_K ? OFF_C1W + o2 * C1_K * C1_K + w2 : OFF_C1B + o2] =
          v;
    } else if (tid >= IB_POOL_T0 && tid < IB_POOL_T0 + 4 * (S1_WSZ + 1)) {
      // four adjacent lanes per pool output, 54 rows each, 2-step shuffle
      const int q = tid - IB_POOL_T0;
      const int w2 = q >> 2;
      const int part = q & 3;
      float s = 0.f;
      if (pool_mode == 0) {
        const float* col =
            rows + part * (S1_OUT / 4) * IB_LD + IB_CONV + w2;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int c = 0; c < S1_OUT / 4; c += 2) {
          s0 += col[(c + 0) * IB_LD];
          s1 += col[(c + 1) * IB_LD];
        }
        s = s0 + s1;
      }
      s += __shfl_xor(s, 1, 4);
      s += __shfl_xor(s, 2, 4);
      IB_STAMP(ST_OWNER);
      if (part == 0)
        out[OFF_S1W + w2] = w2 < S1_WSZ ? s : s * (1.0f / (float)S1_OUT);
    }
    IB_STAMP_DRAIN();
    IB_STAMP(ST_END);
  } else if (MODE == MODE_TRAIN && wgrad_fuse) {
    __syncthreads();
    // conv grads carry the reference 1/(24*24) factor; pool bias /216
    constexpr float inv_pix = 1.0f / (float)C1_PIX;
    if (tid < C1_CH * (C1_K * C1_K + 1)) {
      const int o2 = tid / (C1_K * C1_K + 1);
      const int w2 = tid % (C1_K * C1_K + 1);
      const float v = L.gw[o2][w2] * inv_pix;
      if (w2 < C1_K * C1_K)
        unsafeAtomicAdd(&grads[OFF_C1W + o2 * C1_K * C1_K + w2], v);
      else
        unsafeAtomicAdd(&grads[OFF_C1B + o2], v);
    } else if (pool_mode == 0 &&
               tid < C1_CH * (C1_K * C1_K + 1) + S1_WSZ + 1) {
      const int w2 = tid - C1_CH * (C1_K * C1_K + 1);
      if (w2 < S1_WSZ)
        unsafeAtomicAdd(&grads[OFF_S1W + w2], L.gs1[w2]);
      else
        unsafeAtomicAdd(&grads[OFF_S1B], L.gs1[S1_WSZ] / (float)S1_OUT);
    }
  }
}

// ---------------------------------------------------------------------------
// k_fwdbwd_pair: the in-block training kernel (k_fwdbwd<.., TRAIN, INBLOCK>)
// with TWO adjacent lanes per pool cell and 512-thread blocks, so every SIMD
// holds two waves and the FMA stream issues at the two-wave rate.
//
//   * lane h of a pair computes conv rows 2h, 2h+1 of the cell (8 outputs
//     over a 6x8 window).  Each conv output keeps the cell kernel's FMA
//     order; the pool pre-activation keeps its left-to-right order too: lane
//     0 runs its 8 terms from the bias, hands the running sum to lane 1,
//     which continues with its 8.  a2, y, dz and the loss terms are
//     therefore bit-identical to the cell kernel's.
//   * every load whose address is known at entry is issued before the first
//     conv FMA and held in registers: the fc row slice of the phase-2 lanes,
//     the fc column of the cell, the fc bias, labels[b], the pool weights
//     and bias, the conv weights and bias.  Phase 1 is branch-free (lanes
//     past the last cell redo the last cell and store nothing) and a
//     scheduling barrier closes the load block, so nothing can sink a load
//     below the FMAs; they are consumed once before barrier 1.
//   * conv weight-grad partials are combined across the pair with one
//     xor-1 add per value (both lanes then hold the same sum); each lane
//     stores half of the row: 13 conv sums + its own 8 pool products
//     (+ d2 from lane 1), PR_HALF words per lane at address tid * PR_HALF,
//     an odd stride, so the stores are conflict-free.
//   * owners: two lanes per conv sum (18 cells each), eight per pool sum
//     (27 cells each), fixed order, fixed xor tree.  The slab row differs
//     from the cell kernel's only in summation order.
// ---------------------------------------------------------------------------
constexpr int PR_THREADS = 512;
constexpr int PR_ACTIVE = 2 * S1_OUT;      // 432 lanes own half a cell
constexpr int PR_HALF = 23;                // LDS words per lane
constexpr int PR_LD = 2 * PR_HALF;         // 46 words per cell row
constexpr int PR_CONV_H = IB_CONV / 2;     // 13 conv sums per lane
constexpr int PR_POOL_H = S1_WSZ / 2;      // 8 pool products per lane
constexpr int PR_D2_POS = PR_HALF + PR_CONV_H + PR_POOL_H;  // 44, lane 1
constexpr int PR_CONV_OWNERS = 2 * C1_CH * IB_CONV;         // 312 threads
constexpr int PR_POOL_T0 = 320;            // first pool owner (8-aligned)
constexpr int PR_POOL_LANES = 8;
constexpr int PR_LOSS_T = PR_THREADS - 1;  // wave 7: no cell work in phase 3
static_assert(IB_CONV % 2 == 0 && S1_K % 2 == 0 && PR_HALF % 2 == 1 &&
                  PR_CONV_H + PR_POOL_H + 1 <= PR_HALF &&
                  PR_ACTIVE <= 448 && PR_CONV_OWNERS <= PR_POOL_T0 &&
                  PR_POOL_T0 % PR_POOL_LANES == 0 &&
                  PR_POOL_T0 + PR_POOL_LANES * (S1_WSZ + 1) <= PR_THREADS &&
                  S1_PIX % 2 == 0 && S1_OUT % PR_POOL_LANES == 0 &&
                  FC_OUT * 16 <= PR_THREADS,
              "pair layout");

// Value of the other lane of the pair (lane ^ 1): one DPP quad permute.
__device__ __forceinline__ float pair_other(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(v), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true));
}

template <typename act_t>
__global__ __launch_bounds__(PR_THREADS) void k_fwdbwd_pair(
    const act_t* __restrict__ x, const float* __restrict__ params,
    act_t* __restrict__ a2g, float* __restrict__ yg, float* __restrict__ dzg,
    const int* __restrict__ labels, float* __restrict__ loss_accum, int B,
    int pool_mode, int loss_mode, float* __restrict__ gslab) {
  __shared__ float a2s[S1_OUT];
  __shared__ float ys[FC_OUT];
  __shared__ float dzs[FC_OUT];
  __shared__ float sq[FC_OUT];
  __shared__ float rows[S1_OUT * PR_LD];
  const int b = blockIdx.x;
  if (b >= B) return;
  const int tid = threadIdx.x;
  PCNN_STAMP(ST_ENTRY);
  const bool active = tid < PR_ACTIVE;
  const int cell = active ? tid >> 1 : S1_OUT - 1;
  const int h = tid & 1;
  const int o = cell / S1_PIX;
  const int pq = cell - o * S1_PIX;
  const int pr = pq / S1_W;
  const int pc = pq - pr * S1_W;

  // ---- every load of the kernel, before the first FMA ----
  float xw[6][8];  // rows 2h .. 2h+5 of the cell's 8x8 window
  {
    const act_t* xb = x + (size_t)b * IN_PIX +
                      (pr * S1_K + 2 * h) * IN_W + pc * S1_K;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v4 = 0; v4 < 2; ++v4)
        ld4f(xb + u * IN_W + v4 * 4, &xw[u][v4 * 4]);
  }
  float wv[C1_K * C1_K];
#pragma unroll
  for (int q = 0; q < C1_K * C1_K; ++q)
    wv[q] = params[OFF_C1W + o * C1_K * C1_K + q];
  const float cb = params[OFF_C1B + o];
  float sw[PR_POOL_H];  // pool weights of this lane's two rows
#pragma unroll
  for (int t = 0; t < PR_POOL_H; ++t)
    sw[t] = params[OFF_S1W + h * PR_POOL_H + t];
  const float sb = params[OFF_S1B];
  // phase 2: lane l of class k2 takes a2[l + 16u]; phase 3: the cell's column
  const int k2 = (tid >> 4) < FC_OUT ? (tid >> 4) : FC_OUT - 1;
  const int l = tid & 15;
  constexpr int FC_U = (FC_IN + 15) / 16;  // 14
  float wrow[FC_U];
#pragma unroll
  for (int u = 0; u < FC_U; ++u) {
    const int m = l + u * 16;
    wrow[u] = params[OFF_FW + k2 * FC_IN + (m < FC_IN ? m : FC_IN - 1)];
  }
  const float fb = params[OFF_FB + k2];
  float fcol[FC_OUT];
#pragma unroll
  for (int k = 0; k < FC_OUT; ++k)
    fcol[k] = params[OFF_FW + k * FC_IN + cell];
  const int lab = labels[b];
  __builtin_amdgcn_sched_barrier(0);
  PCNN_STAMP_DRAIN();
  PCNN_STAMP(ST_LOADS);

  // ---- phase 1: conv1 + sigmoid + pool + sigmoid ----
  float av[2 * S1_K];  // this lane's 8 conv activations, kept live to bwd
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < S1_K; ++j) {
      float acc = cb;
#pragma unroll
      for (int u = 0; u < C1_K; ++u)
#pragma unroll
        for (int v = 0; v < C1_K; ++v)
          acc = __builtin_fmaf(wv[u * C1_K + v], xw[i + u][j + v], acc);
      av[i * S1_K + j] = sigmoidf_dev(acc);
    }
  }
  // pool preact in the cell kernel's order: lane 0's 8 terms from the bias
  // (or the max identity), then lane 1's 8 on top of lane 0's running value
  float p0 = pool_mode == 1 ? -1e30f : sb;
#pragma unroll
  for (int t = 0; t < 2 * S1_K; ++t) {
    if (pool_mode == 1)
      p0 = fmaxf(p0, av[t]);
    else
      p0 = __builtin_fmaf(sw[t], av[t], p0);
  }
  float p1 = pair_other(p0);  // meaningful in lane 1: lane 0's sum
#pragma unroll
  for (int t = 0; t < 2 * S1_K; ++t) {
    if (pool_mode == 1)
      p1 = fmaxf(p1, av[t]);
    else
      p1 = __builtin_fmaf(sw[t], av[t], p1);
  }
  const float p1o = pair_other(p1);
  const float a2v = sigmoidf_dev(h ? p1 : p1o);
  if (active && h == 0) {
    a2s[cell] = a2v;
    stf(a2g + (size_t)b * S1_OUT + cell, a2v);
  }
  // the hoisted values are consumed here, so their loads stay above
#pragma unroll
  for (int u = 0; u < FC_U; ++u) asm volatile("" : "+v"(wrow[u]));
#pragma unroll
  for (int k = 0; k < FC_OUT; ++k) asm volatile("" : "+v"(fcol[k]));
  PCNN_STAMP(ST_CONV);
  __syncthreads();
  PCNN_STAMP(ST_BAR1);

  // ---- phase 2: fc (216 -> 10) + sigmoid + residual, as the cell kernel ----
  if (tid < FC_OUT * 16) {
    const int k = tid >> 4;
    float p = 0.f;
#pragma unroll
    for (int u = 0; u < FC_U; ++u) {
      const int m = l + u * 16;
      if (m < FC_IN) p = __builtin_fmaf(wrow[u], a2s[m], p);
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) p += __shfl_down(p, off, 16);
    if (l == 0) {
      const float z = p + fb;
      if (loss_mode == 1) {
        ys[k] = z;  // raw logit; softmax finished below
      } else {
        const float v = sigmoidf_dev(z);
        ys[k] = v;
        if (yg != nullptr) yg[(size_t)b * FC_OUT + k] = v;
        const float d = (k == lab ? 1.0f : 0.0f) - v;
        dzs[k] = d;
        sq[k] = d * d;
        dzg[(size_t)b * FC_OUT + k] = d;
      }
    }
  }
  PCNN_STAMP(ST_FC);
  __syncthreads();
  if (loss_mode == 1) {
    if (tid == 0) {
      float mx = ys[0];
#pragma unroll
      for (int k = 1; k < FC_OUT; ++k) mx = fmaxf(mx, ys[k]);
      float sum = 0.f;
      float e[FC_OUT];
#pragma unroll
      for (int k = 0; k < FC_OUT; ++k) {
        e[k] = __expf(ys[k] - mx);
        sum += e[k];
      }
#pragma unroll
      for (int k = 0; k < FC_OUT; ++k) {
        const float v = e[k] / sum;
        ys[k] = v;
        if (yg != nullptr) yg[(size_t)b * FC_OUT + k] = v;
        const float d = (k == lab ? 1.0f : 0.0f) - v;
        dzs[k] = d;
        dzg[(size_t)b * FC_OUT + k] = d;
      }
      sq[0] = -__logf(fmaxf(ys[lab], 1e-30f));
    }
    __syncthreads();
  }
  PCNN_STAMP(ST_BAR2);

  // ---- phase 3: fc bwd -> pool bwd -> weight-grad partials ----
  if (tid < 448) {  // wave-uniform: waves 0-6 hold the 432 pair lanes
    float da = 0.f;
#pragma unroll
    for (int k = 0; k < FC_OUT; ++k) da = __builtin_fmaf(fcol[k], dzs[k], da);
    const float d2 = da * a2v * (1.0f - a2v);
    // max pooling: d2 goes to the cell's first maximum; the pair settles
    // which lane holds it (lane 0 wins ties, as the ascending scan does)
    int best = -1;
    if (pool_mode == 1) {
      float bv = av[0];
      int bi = 0;
#pragma unroll
      for (int t = 1; t < 2 * S1_K; ++t)
        if (av[t] > bv) {
          bv = av[t];
          bi = t;
        }
      const float ov = pair_other(bv);
      const bool mine = h ? (bv > ov) : !(ov > bv);
      best = mine ? bi : -1;
    }
    float dz1v[2 * S1_K];
#pragma unroll
    for (int t = 0; t < 2 * S1_K; ++t) {
      const float a = av[t];
      const float dd = pool_mode == 1 ? (t == best ? d2 : 0.f) : d2 * sw[t];
      dz1v[t] = dd * a * (1.0f - a);
    }
    PCNN_STAMP(ST_BWD);
    // conv1 partial of this half cell: 8 dz1 x the 6x8 window (200 FMAs).
    // dz1 and a1 enter rounded to the activation dtype, as in the cell
    // kernel.
    float cacc[C1_K * C1_K];
#pragma unroll
    for (int w2 = 0; w2 < C1_K * C1_K; ++w2) cacc[w2] = 0.f;
    float csum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < S1_K; ++j) {
        const float d = (float)(act_t)dz1v[i * S1_K + j];
        csum += d;
#pragma unroll
        for (int u = 0; u < C1_K; ++u)
#pragma unroll
          for (int v = 0; v < C1_K; ++v)
            cacc[u * C1_K + v] += d * xw[i + u][j + v];
      }
    // pair sum: a + b is the same number in both lanes
#pragma unroll
    for (int w2 = 0; w2 < C1_K * C1_K; ++w2) cacc[w2] += pair_other(cacc[w2]);
    csum += pair_other(csum);
    PCNN_STAMP(ST_WGRAD);
    if (active) {
      float* row = rows + tid * PR_HALF;
#pragma unroll
      for (int s = 0; s < PR_CONV_H; ++s) {
        const float hi = PR_CONV_H + s < C1_K * C1_K ? cacc[PR_CONV_H + s]
                                                     : csum;
        row[s] = h ? hi : cacc[s];
      }
      if (pool_mode == 0) {
#pragma unroll
        for (int t = 0; t < PR_POOL_H; ++t)
          row[PR_CONV_H + t] = d2 * (float)(act_t)av[t];
        if (h) row[PR_CONV_H + PR_POOL_H] = d2;
      }
    }
    PCNN_STAMP_LDS_DRAIN();
    PCNN_STAMP(ST_LDS);
  } else if (tid == PR_LOSS_T && loss_accum != nullptr) {
    if (loss_mode == 1) {
      unsafeAtomicAdd(loss_accum, sq[0]);
    } else {
      float ssum = 0.f;
#pragma unroll
      for (int k = 0; k < FC_OUT; ++k) ssum += sq[k];
      unsafeAtomicAdd(loss_accum, sqrtf(ssum));
    }
  }
  __syncthreads();
  PCNN_STAMP(ST_BAR3);

  // ---- owners: fixed-order sums over the 216 cell rows ----
  float* out = gslab + (size_t)b * GSLAB_LD;
  if (tid < PR_CONV_OWNERS) {
    // two lanes per (channel, 5x5 weight | bias), 18 of the 36 cells each
    const int own = tid >> 1;
    const int o2 = own / IB_CONV;
    const int w2 = own - o2 * IB_CONV;
    const int pos = w2 < PR_CONV_H ? w2 : PR_HALF + w2 - PR_CONV_H;
    const float* col = rows + (o2 * S1_PIX + h * (S1_PIX / 2)) * PR_LD + pos;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < S1_PIX / 2; c += 3) {
      s0 += col[(c + 0) * PR_LD];
      s1 += col[(c + 1) * PR_LD];
      s2 += col[(c + 2) * PR_LD];
    }
    float s = (s0 + s1) + s2;
    s += pair_other(s);
    PCNN_STAMP(ST_OWNER);
    if (h == 0)
      out[w2 < C1_K * C1_K ? OFF_C1W + o2 * C1_K * C1_K + w2 : OFF_C1B + o2] =
          s * (1.0f / (float)C1_PIX);
  } else if (tid >= PR_POOL_T0 &&
             tid < PR_POOL_T0 + PR_POOL_LANES * (S1_WSZ + 1)) {
    // eight adjacent lanes per pool output, 27 cell rows each
    const int q = tid - PR_POOL_T0;
    const int w2 = q >> 3;
    const int part = q & (PR_POOL_LANES - 1);
    constexpr int RP = S1_OUT / PR_POOL_LANES;  // 27
    float s = 0.f;
    if (pool_mode == 0) {
      const int pos = w2 < S1_WSZ
                          ? (w2 / PR_POOL_H) * PR_HALF + PR_CONV_H +
                                w2 % PR_POOL_H
                          : PR_D2_POS;
      const float* col = rows + part * RP * PR_LD + pos;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int c = 0; c < RP; c += 3) {
        s0 += col[(c + 0) * PR_LD];
        s1 += col[(c + 1) * PR_LD];
        s2 += col[(c + 2) * PR_LD];
      }
      s = (s0 + s1) + s2;
    }
    s += __shfl_xor(s, 1, PR_POOL_LANES);
    s += __shfl_xor(s, 2, PR_POOL_LANES);
    s += __shfl_xor(s, 4, PR_POOL_LANES);
    PCNN_STAMP(ST_OWNER);
    if (part == 0)
      out[OFF_S1W + w2] = w2 < S1_WSZ ? s : s * (1.0f / (float)S1_OUT);
  }
  PCNN_STAMP_DRAIN();
  PCNN_STAMP(ST_END);
}

// ---------------------------------------------------------------------------
// Weight gradients, batch-reduced (v2 — barrier-free grid-stride).
//
// Grid role layout (GC = blocks per conv channel, GS = pool blocks):
//   blocks [0, 6*GC)            : conv1 wgrad+bgrad, blk -> (channel, slice)
//   blocks [6*GC, 6*GC+GS)      : pool wgrad+bgrad
//   blocks [6*GC+GS, +9)        : fc wgrad+bgrad (2160 weights + 10 biases,
//                                 one owner thread each — no atomics)
// ---------------------------------------------------------------------------

constexpr int WG_GC_DEFAULT = 8;   // conv1 slices per channel (runtime knob)
constexpr int FC_BLOCKS = (FC_WSZ + 255) / 256;  // 9

// Cross-lane sum over the full 64-lane wave.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The whole role dispatch lives in one device function so that the plain
// kernel and the update-fused kernel below run the very same gradient code.
// A masked-off role returns from this function only, never from the kernel.
//
// WT (update-fused kernel only): the fc role's owner stores are agent-scope
// write-through stores instead of plain ones, so that — like the conv and
// pool roles' hardware atomics — they have left this XCD's L2 once the
// storing wave's vmcnt has drained, and the hand-off to the block that
// applies the update needs no L2 write-back.
template <typename act_t, bool WT>
__device__ __forceinline__ void wgrad_body(
    const act_t* __restrict__ x, const act_t* __restrict__ a1g,
    const act_t* __restrict__ a2g, const float* __restrict__ dzg,
    const float* __restrict__ dz2g, const act_t* __restrict__ dz1g,
    float* __restrict__ grads, int B, int GC, int GS, int FS, int roles) {
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  const int lane = tid & 63;

  if (blk < C1_CH * GC) {
    if (!(roles & 1)) return;
    // ---- conv1: dW[o,i,j] = sum_{b,r,c} dz1[b,o,r,c] * x[b,r+i,c+j] / 576
    // Work item = 4 consecutive output columns of one row: 5 vectorized
    // 8-wide x row loads + one float4 dz1 load replace 104 scalar loads
    // (the v2 scalar form was address-issue-bound: profiles/ r1).  Two
    // groups are processed per loop iteration so the second group's loads
    // issue before the first group's FMAs — one memory-latency stall per
    // TWO groups instead of one per group.
    const int o = blk / GC;
    const int slice = blk - o * GC;
    constexpr int GROUPS_PER_ROW = C1_W / 4;  // 6
    float acc[C1_K * C1_K];
#pragma unroll
    for (int w = 0; w < C1_K * C1_K; ++w) acc[w] = 0.f;
    float bacc = 0.f;
    const int N = B * C1_H * GROUPS_PER_ROW;
    const int stride = GC * 256;
    for (int it = slice * 256 + tid; it < N; it += 2 * stride) {
      const int it2 = it + stride;
      float d4a[4], xra[C1_K][8];
      float d4b[4], xrb[C1_K][8];
      {
        const int bi = it / (C1_H * GROUPS_PER_ROW);
        const int rg = it - bi * (C1_H * GROUPS_PER_ROW);
        const int r = rg / GROUPS_PER_ROW;
        const int c0 = (rg - r * GROUPS_PER_ROW) * 4;
        ld4f(dz1g + (size_t)bi * C1_OUT + o * C1_PIX + r * C1_W + c0, d4a);
        const act_t* xb = x + (size_t)bi * IN_PIX + r * IN_W + c0;
#pragma unroll
        for (int i = 0; i < C1_K; ++i) ld8f(xb + i * IN_W, xra[i]);
      }
      if (it2 < N) {
        const int bi = it2 / (C1_H * GROUPS_PER_ROW);
        const int rg = it2 - bi * (C1_H * GROUPS_PER_ROW);
        const int r = rg / GROUPS_PER_ROW;
        const int c0 = (rg - r * GROUPS_PER_ROW) * 4;
        ld4f(dz1g + (size_t)bi * C1_OUT + o * C1_PIX + r * C1_W + c0, d4b);
        const act_t* xb = x + (size_t)bi * IN_PIX + r * IN_W + c0;
#pragma unroll
        for (int i = 0; i < C1_K; ++i) ld8f(xb + i * IN_W, xrb[i]);
      }
      bacc += d4a[0] + d4a[1] + d4a[2] + d4a[3];
#pragma unroll
      for (int i = 0; i < C1_K; ++i)
#pragma unroll
        for (int pp = 0; pp < 4; ++pp)
#pragma unroll
          for (int j = 0; j < C1_K; ++j)
            acc[i * C1_K + j] += d4a[pp] * xra[i][pp + j];
      if (it2 < N) {
        bacc += d4b[0] + d4b[1] + d4b[2] + d4b[3];
#pragma unroll
        for (int i = 0; i < C1_K; ++i)
#pragma unroll
          for (int pp = 0; pp < 4; ++pp)
#pragma unroll
            for (int j = 0; j < C1_K; ++j)
              acc[i * C1_K + j] += d4b[pp] * xrb[i][pp + j];
      }
    }
    // cross-wave pre-reduce in LDS: one hardware atomic per weight per
    // BLOCK (was one per wave -> 4x the same-address atomic traffic).
    __shared__ float red[4][C1_K * C1_K + 1];
    const int wv = tid >> 6;
#pragma unroll
    for (int w = 0; w < C1_K * C1_K; ++w) {
      const float v = wave_sum(acc[w]);
      if (lane == 0) red[wv][w] = v;
    }
    {
      const float v = wave_sum(bacc);
      if (lane == 0) red[wv][C1_K * C1_K] = v;
    }
    __syncthreads();
    constexpr float inv_pix = 1.0f / (float)C1_PIX;
    if (tid < C1_K * C1_K) {
      const float v =
          red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      unsafeAtomicAdd(&grads[OFF_C1W + o * C1_K * C1_K + tid], v * inv_pix);
    } else if (tid == C1_K * C1_K) {
      const float v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      unsafeAtomicAdd(&grads[OFF_C1B + o], v * inv_pix);
    }
  } else if (blk < C1_CH * GC + GS) {
    if (!(roles & 2)) return;
    // ---- pool: dW[i,j] = sum_{b,o,p,q} dz2[b,o,p,q] * a1[b,o,4p+i,4q+j]
    const int slice = blk - C1_CH * GC;
    float acc[S1_WSZ];
#pragma unroll
    for (int w = 0; w < S1_WSZ; ++w) acc[w] = 0.f;
    float bacc = 0.f;
    const int N = B * S1_OUT;
    const int stride = GS * 256;
    for (int it = slice * 256 + tid; it < N; it += 2 * stride) {
      const int it2 = it + stride;
      float da = 0.f, db = 0.f, ara[S1_K][S1_K], arb[S1_K][S1_K];
      {
        const int bi = it / S1_OUT;
        const int opq = it - bi * S1_OUT;
        const int oo = opq / S1_PIX;
        const int pq = opq - oo * S1_PIX;
        const int prr = pq / S1_W;
        const int pcc = pq - prr * S1_W;
        da = dz2g[it];
        const act_t* base = a1g + (size_t)bi * C1_OUT + oo * C1_PIX +
                            prr * S1_K * C1_W + pcc * S1_K;
#pragma unroll
        for (int i = 0; i < S1_K; ++i) ld4f(base + i * C1_W, ara[i]);
      }
      if (it2 < N) {
        const int bi = it2 / S1_OUT;
        const int opq = it2 - bi * S1_OUT;
        const int oo = opq / S1_PIX;
        const int pq = opq - oo * S1_PIX;
        const int prr = pq / S1_W;
        const int pcc = pq - prr * S1_W;
        db = dz2g[it2];
        const act_t* base = a1g + (size_t)bi * C1_OUT + oo * C1_PIX +
                            prr * S1_K * C1_W + pcc * S1_K;
#pragma unroll
        for (int i = 0; i < S1_K; ++i) ld4f(base + i * C1_W, arb[i]);
      }
      bacc += da;
#pragma unroll
      for (int i = 0; i < S1_K; ++i)
#pragma unroll
        for (int j = 0; j < S1_K; ++j) acc[i * S1_K + j] += da * ara[i][j];
      if (it2 < N) {
        bacc += db;
#pragma unroll
        for (int i = 0; i < S1_K; ++i)
#pragma unroll
          for (int j = 0; j < S1_K; ++j) acc[i * S1_K + j] += db * arb[i][j];
      }
    }
    __shared__ float red[4][S1_WSZ + 1];
    const int wv = tid >> 6;
#pragma unroll
    for (int w = 0; w < S1_WSZ; ++w) {
      const float v = wave_sum(acc[w]);
      if (lane == 0) red[wv][w] = v;
    }
    {
      const float v = wave_sum(bacc);
      if (lane == 0) red[wv][S1_WSZ] = v;
    }
    __syncthreads();
    if (tid < S1_WSZ) {
      const float v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      unsafeAtomicAdd(&grads[OFF_S1W + tid], v);
    } else if (tid == S1_WSZ) {
      const float v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
      unsafeAtomicAdd(&grads[OFF_S1B], v / (float)S1_OUT);
    }
  } else {
    if (!(roles & 4)) return;
    // ---- fc: dW[k,m] = sum_b dz[b,k] * a2[b,m];  db[k] = sum_b dz[b,k]
    // FS batch slices; one owner thread per (weight, slice).  With FS==1
    // the owner accumulates with a plain store (no atomics); FS>1 (large
    // batch) uses hardware atomics across slices.
    const int fblk = blk - C1_CH * GC - GS;
    const int slice = fblk / FC_BLOCKS;
    const int q = (fblk - slice * FC_BLOCKS) * 256 + tid;
    const int b_lo = (int)(((long)B * slice) / FS);
    const int b_hi = (int)(((long)B * (slice + 1)) / FS);
    if (q < FC_WSZ) {
      const int k = q / FC_IN;
      const int m = q - k * FC_IN;
      float acc = 0.f;
#pragma unroll 8
      for (int b = b_lo; b < b_hi; ++b)
        acc += dzg[(size_t)b * FC_OUT + k] * ldf(a2g + (size_t)b * FC_IN + m);
      if (FS == 1 && WT)
        __hip_atomic_store(&grads[OFF_FW + q], grads[OFF_FW + q] + acc,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else if (FS == 1)
        grads[OFF_FW + q] += acc;
      else
        unsafeAtomicAdd(&grads[OFF_FW + q], acc);
    } else if (q < FC_WSZ + FC_OUT) {
      const int k = q - FC_WSZ;
      float acc = 0.f;
#pragma unroll 8
      for (int b = b_lo; b < b_hi; ++b) acc += dzg[(size_t)b * FC_OUT + k];
      if (FS == 1 && WT)
        __hip_atomic_store(&grads[OFF_FB + k], grads[OFF_FB + k] + acc,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else if (FS == 1)
        grads[OFF_FB + k] += acc;
      else
        unsafeAtomicAdd(&grads[OFF_FB + k], acc);
    }
  }
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_wgrad(
    const act_t* __restrict__ x, const act_t* __restrict__ a1g,
    const act_t* __restrict__ a2g, const float* __restrict__ dzg,
    const float* __restrict__ dz2g, const act_t* __restrict__ dz1g,
    float* __restrict__ grads, int B, int GC, int GS, int FS, int roles) {
  wgrad_body<act_t, false>(x, a1g, a2g, dzg, dz2g, dz1g, grads, B, GC, GS,
                           FS, roles);
}

// ---------------------------------------------------------------------------
// Arrival ticket: every block of a launch arrives exactly once and exits;
// nothing waits.  Returns true (block-uniform) in the block that arrived
// last, after which that block may read everything the other blocks wrote
// before they arrived.
//
// Publish side: everything a block hands over is written with agent-scope
// atomics or agent-scope write-through stores (never plain stores), so it
// has left the XCD's L2 once the writing wave's vmcnt has drained; every
// wave drains, the block meets at a barrier, then one lane draws a ticket
// with a returning agent-scope atomic.  An agent-scope release fence (an
// L2 write-back, ~1.7 us in every block) in front of the ticket measured
// 19.0 us/step against 18.6 for three launches, which is why the payload
// is write-through instead.  Consume side: the lane that drew gridDim.x-1
// does an agent-scope acquire and drains it before the barrier that lets
// the other waves load.  Visibility therefore never depends on which XCD
// a block ran on.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool arrive_is_last(int* __restrict__ ticket) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    const int last = (t == (int)gridDim.x - 1);
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_last = last;
  }
  __syncthreads();
  return s_last != 0;
}

// SGD apply + gradient zeroing over the whole bucket by ONE 256-thread
// block (the last arriver): sgd_apply4 / sgd_apply1 in the same float4 split
// as k_update, 585 vectors + a 3-float scalar tail.  Under OPT_MOM the block
// is the only reader and writer of vel in the launch.  vel was written by
// the last arriver of the previous launch with plain stores and has crossed
// a kernel boundary since, exactly like params: plain loads and stores, no
// fences beyond the ticket's.  The same holds for Adam's two buckets (m in
// vel, s in sq) under OPT_ADAM.
template <int OPT, typename Args>
__device__ __forceinline__ void update_tail(float* __restrict__ params,
                                            float* __restrict__ grads,
                                            float* __restrict__ vel,
                                            float* __restrict__ sq,
                                            float step, const Args& o) {
  constexpr int NV = N_PARAMS / 4;
  for (int i4 = threadIdx.x; i4 < NV; i4 += 256)
    sgd_apply4<OPT>(params, grads, vel, sq, i4 * 4, step, o);
  const int u = NV * 4 + threadIdx.x;
  if (u < N_PARAMS) sgd_apply1<OPT>(params, grads, vel, sq, u, step, o);
}

// Weight gradients with the SGD update as the tail of the same launch
// (two-launch training step).  Gradient code is wgrad_body, unchanged; the
// block that arrives last applies the update, zeroes the bucket and resets
// the ticket for the next launch.
template <typename act_t, int OPT, typename Args>
__device__ __forceinline__ void wgrad_update_body(
    const act_t* __restrict__ x, const act_t* __restrict__ a1g,
    const act_t* __restrict__ a2g, const float* __restrict__ dzg,
    const float* __restrict__ dz2g, const act_t* __restrict__ dz1g,
    float* __restrict__ grads, int B, int GC, int GS, int FS, int roles,
    float* __restrict__ params, float step, float* __restrict__ vel,
    float* __restrict__ sq, const Args& o, int* __restrict__ ticket) {
  wgrad_body<act_t, true>(x, a1g, a2g, dzg, dz2g, dz1g, grads, B, GC, GS,
                          FS, roles);
  if (!arrive_is_last(ticket)) return;
  update_tail<OPT>(params, grads, vel, sq, step, o);
  if (threadIdx.x == 0)
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_wgrad_update_mom(
    const act_t* __restrict__ x, const act_t* __restrict__ a1g,
    const act_t* __restrict__ a2g, const float* __restrict__ dzg,
    const float* __restrict__ dz2g, const act_t* __restrict__ dz1g,
    float* __restrict__ grads, int B, int GC, int GS, int FS, int roles,
    float* __restrict__ params, float* __restrict__ vel, MomArgs o,
    int* __restrict__ ticket) {
  wgrad_update_body<act_t, OPT_MOM>(x, a1g, a2g, dzg, dz2g, dz1g, grads, B,
                                    GC, GS, FS, roles, params, 0.f, vel,
                                    nullptr, o, ticket);
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_wgrad_update_adam(
    const act_t* __restrict__ x, const act_t* __restrict__ a1g,
    const act_t* __restrict__ a2g, const float* __restrict__ dzg,
    const float* __restrict__ dz2g, const act_t* __restrict__ dz1g,
    float* __restrict__ grads, int B, int GC, int GS, int FS, int roles,
    float* __restrict__ params, float* __restrict__ vel,
    float* __restrict__ sq, AdamArgs o, int* __restrict__ ticket) {
  wgrad_update_body<act_t, OPT_ADAM>(x, a1g, a2g, dzg, dz2g, dz1g, grads, B,
                                     GC, GS, FS, roles, params, 0.f, vel, sq,
                                     o, ticket);
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_wgrad_update(
    const act_t* __restrict__ x, const act_t* __restrict__ a1g,
    const act_t* __restrict__ a2g, const float* __restrict__ dzg,
    const float* __restrict__ dz2g, const act_t* __restrict__ dz1g,
    float* __restrict__ grads, int B, int GC, int GS, int FS, int roles,
    float* __restrict__ params, float step, int* __restrict__ ticket) {
  wgrad_update_body<act_t, OPT_PLAIN>(x, a1g, a2g, dzg, dz2g, dz1g, grads, B,
                                      GC, GS, FS, roles, params, step,
                                      nullptr, nullptr, MomArgs{}, ticket);
}

// ---------------------------------------------------------------------------
// SGD apply + gradient zeroing as a launch of its own: one float4 per thread
// across the grid (the bucket is 16B-aligned), scalar tail.
// ---------------------------------------------------------------------------
template <int OPT, typename Args>
__device__ __forceinline__ void update_body(float* __restrict__ params,
                                            float* __restrict__ grads,
                                            float* __restrict__ vel,
                                            float* __restrict__ sq,
                                            float step, const Args& o) {
  const int i4 = blockIdx.x * 256 + threadIdx.x;
  const int i = i4 * 4;
  if (i + 3 < N_PARAMS) {
    sgd_apply4<OPT>(params, grads, vel, sq, i, step, o);
  } else if (i < N_PARAMS) {
    for (int u = i; u < N_PARAMS; ++u)
      sgd_apply1<OPT>(params, grads, vel, sq, u, step, o);
  }
}

__global__ __launch_bounds__(256) void k_update(float* __restrict__ params,
                                                float* __restrict__ grads,
                                                float step) {
  update_body<OPT_PLAIN>(params, grads, nullptr, nullptr, step, MomArgs{});
}

__global__ __launch_bounds__(256) void k_update_mom(
    float* __restrict__ params, float* __restrict__ grads,
    float* __restrict__ vel, MomArgs o) {
  update_body<OPT_MOM>(params, grads, vel, nullptr, 0.f, o);
}

__global__ __launch_bounds__(256) void k_update_adam(
    float* __restrict__ params, float* __restrict__ grads,
    float* __restrict__ vel, float* __restrict__ sq, AdamArgs o) {
  update_body<OPT_ADAM>(params, grads, vel, sq, 0.f, o);
}


// ---------------------------------------------------------------------------
// Second kernel of the in-block weight-grad step: batch-reduce + SGD apply.
// Every parameter has exactly one owner group of RU_LANES adjacent lanes, so
// there are no atomics, no gradient bucket, no ticket and no fences:
//   p <  173        g = sum_b gslab[b][p]           (scaled by the writer)
//   fc weight (k,m) g = sum_b dz[b][k] * a2[b][m]
//   fc bias k       g = sum_b dz[b][k]
//   params[p] += step * g
// Lane `sub` of a group takes images sub, sub+4, ...  Each lane adds in
// ascending image order into one accumulator and the group combines with a
// fixed 2-step xor shuffle, so the result does not depend on which block ran
// where or when.
//
// The kernel is one dependent chain, so what it costs is the number of
// memory round trips on that chain, and it is written to have one at B <= 64:
//   * every kernel argument is fetched at entry, behind one scalar wait;
//   * params[p] (and vel[p], sq[p]) are loaded at entry, with the clamped
//     index, next to the first batch loads, not after the shuffle;
//   * the three cases are one branch-free path: a column pointer and a row
//     stride select slab column or dz column, and a lane that is not an fc
//     weight multiplies by 1.0f (fma(d, 1, acc) is d + acc, bit for bit), so
//     a wave that straddles two cases does not run two load chains;
//   * a trip is RU_LANES * DEPTH images, loaded with clamped addresses and a
//     select so the loads stay unconditional; the loads of trip t+1 are
//     issued before the adds of trip t (trip count is block-uniform).  The
//     compiler gives trip t+1 the registers of trip t, so those loads still
//     wait for the oldest data of trip t: B = 256 is about four round trips.
//     DEPTH is 16, so B <= 64 is a single trip, but 8 up to 32 images:
//     with depth 16 at B = 16, 24 of a lane's 32 loads are clamped repeats
//     and the step is 0.27 us slower (8.95 against 8.67, the whole gain at
//     that size; profiles/r8).
// ---------------------------------------------------------------------------
constexpr int RU_LANES = 4;
constexpr int RU_DEPTH_SMALL = 8;   // B <= RU_LANES * RU_DEPTH_SMALL
constexpr int RU_DEPTH = 16;
constexpr int RU_PARAMS_PER_BLOCK = 256 / RU_LANES;  // 64
constexpr int RU_BLOCKS =
    (N_PARAMS + RU_PARAMS_PER_BLOCK - 1) / RU_PARAMS_PER_BLOCK;  // 37
// Largest batch the step launcher gives to this pair of kernels (measured
// crossover: pcnn_launch_step_inblock).
constexpr int INBLOCK_MAX_B = 256;
// Kernel 1 of the in-block step when the caller does not choose: 0 = cell
// (k_fwdbwd<.., INBLOCK>), 1 = pair (k_fwdbwd_pair).
constexpr int INBLOCK_DEFAULT_VARIANT = 1;

// Have the optimizer's kernel arguments in scalar registers here (an empty
// statement that reads them): one fetch at entry instead of one per use.
__device__ __forceinline__ void ru_fetch_args(const MomArgs& o) {
  asm volatile("" ::"s"(o.scale), "s"(o.dt), "s"(o.mu), "s"(o.wd),
               "s"(o.nesterov));
}
__device__ __forceinline__ void ru_fetch_args(const AdamArgs& o) {
  asm volatile("" ::"s"(o.scale), "s"(o.dt), "s"(o.beta1), "s"(o.beta2),
               "s"(o.eps), "s"(o.wd), "s"(o.c1), "s"(o.c2), "s"(o.omb1),
               "s"(o.omb2));
}

// One trip of a lane: images b0, b0 + 4, ..., DEPTH of them.  ru_load only
// issues the loads (clamped, so unconditional); ru_add applies the selects,
// d = 0 past the batch and a = 1.0f outside the fc weights, where it adds, so
// nothing in a load block waits for data.
template <int DEPTH, typename act_t>
__device__ __forceinline__ void ru_load(float (&d)[DEPTH], act_t (&a)[DEPTH],
                                        const float* __restrict__ dcol,
                                        int dld,
                                        const act_t* __restrict__ acol,
                                        int b0, int B) {
#pragma unroll
  for (int u = 0; u < DEPTH; ++u) {
    const int b = b0 + u * RU_LANES;
    const int bc = b < B ? b : B - 1;
    d[u] = dcol[(size_t)bc * dld];
    a[u] = acol[(size_t)bc * FC_IN];
  }
}
template <int DEPTH, typename act_t>
__device__ __forceinline__ float ru_add(float acc, const float (&d)[DEPTH],
                                        const act_t (&a)[DEPTH], bool fcw,
                                        int b0, int B) {
#pragma unroll
  for (int u = 0; u < DEPTH; ++u)
    acc = __builtin_fmaf(b0 + u * RU_LANES < B ? d[u] : 0.f,
                         fcw ? (float)a[u] : 1.0f, acc);
  return acc;
}

// Sum of one lane over its images, ascending, into one accumulator.
template <int DEPTH, typename act_t>
__device__ __forceinline__ float ru_sum(const float* __restrict__ dcol,
                                        int dld,
                                        const act_t* __restrict__ acol,
                                        bool fcw, int sub, int B) {
  constexpr int STEP_B = RU_LANES * DEPTH;
  float d[DEPTH];
  act_t a[DEPTH];
  ru_load<DEPTH>(d, a, dcol, dld, acol, sub, B);
  __builtin_amdgcn_sched_barrier(0);
  float acc = 0.f;
  int base = 0;  // first image of the trip in d, a: block-uniform
  for (; base + STEP_B < B; base += STEP_B) {
    float dn[DEPTH];
    act_t an[DEPTH];
    ru_load<DEPTH>(dn, an, dcol, dld, acol, base + STEP_B + sub, B);
    __builtin_amdgcn_sched_barrier(0);
    acc = ru_add<DEPTH>(acc, d, a, fcw, base + sub, B);
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      d[u] = dn[u];
      a[u] = an[u];
    }
  }
  return ru_add<DEPTH>(acc, d, a, fcw, base + sub, B);
}

// OPT selects the apply at the end and nothing else: the plain kernel is the
// OPT_PLAIN instantiation with vel, sq and o unused; the momentum and Adam
// kernels have the owner lane (sub == 0) do the read-modify-write of their
// state (vel; m in vel and s in sq) and the parameter store after the same
// fixed shuffle.
template <typename act_t, int OPT, typename Args>
__device__ __forceinline__ void reduce_update_body(
    const float* __restrict__ gslab, const act_t* __restrict__ a2g,
    const float* __restrict__ dzg, float* __restrict__ params, float step,
    int B, float* __restrict__ vel, float* __restrict__ sq, const Args& o) {
  asm volatile("" ::"s"(gslab), "s"(a2g), "s"(dzg), "s"(params), "s"(B));
  if constexpr (OPT == OPT_PLAIN) asm volatile("" ::"s"(step));
  if constexpr (OPT != OPT_PLAIN) {
    asm volatile("" ::"s"(vel));
    ru_fetch_args(o);
  }
  if constexpr (OPT == OPT_ADAM) asm volatile("" ::"s"(sq));
  const int p = blockIdx.x * RU_PARAMS_PER_BLOCK + (threadIdx.x >> 2);
  const int sub = threadIdx.x & (RU_LANES - 1);
  // Lanes past the last parameter redo the last one and do not store: the
  // whole group stays active for the shuffle.
  const int pc = p < N_PARAMS ? p : N_PARAMS - 1;
  // state of the parameter, in flight together with the first batch loads
  float pv = params[pc];
  float mv = 0.f, sv = 0.f;
  if constexpr (OPT != OPT_PLAIN) mv = vel[pc];
  if constexpr (OPT == OPT_ADAM) sv = sq[pc];
  // slab column pc | dz column k of fc weight (k, m) | dz column of fc bias
  const bool slab = pc < OFF_FW;
  const bool fcw = !slab && pc < OFF_FB;
  const int q = fcw ? pc - OFF_FW : 0;
  const int k = fcw ? q / FC_IN : (slab ? 0 : pc - OFF_FB);
  const int m = q - (fcw ? k : 0) * FC_IN;
  const float* dcol = slab ? gslab + pc : dzg + k;
  const int dld = slab ? GSLAB_LD : FC_OUT;
  const act_t* acol = a2g + m;
  float acc = B <= RU_LANES * RU_DEPTH_SMALL
                  ? ru_sum<RU_DEPTH_SMALL>(dcol, dld, acol, fcw, sub, B)
                  : ru_sum<RU_DEPTH>(dcol, dld, acol, fcw, sub, B);
  // consumed here, by every lane, so the state loads stay at the top
  asm volatile("" : "+v"(pv));
  if constexpr (OPT != OPT_PLAIN) asm volatile("" : "+v"(mv));
  if constexpr (OPT == OPT_ADAM) asm volatile("" : "+v"(sv));
  acc += __shfl_xor(acc, 1, RU_LANES);
  acc += __shfl_xor(acc, 2, RU_LANES);
  if (sub == 0 && p < N_PARAMS) {
    if constexpr (OPT == OPT_ADAM) {
      params[p] = adam_apply(pv, acc, mv, sv, o);
      vel[p] = mv;
      sq[p] = sv;
    } else if constexpr (OPT == OPT_MOM) {
      params[p] = mom_apply(pv, acc, mv, o);
      vel[p] = mv;
    } else {
      params[p] = __builtin_fmaf(step, acc, pv);
    }
  }
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_reduce_update(
    const float* __restrict__ gslab, const act_t* __restrict__ a2g,
    const float* __restrict__ dzg, float* __restrict__ params, float step,
    int B) {
  reduce_update_body<act_t, OPT_PLAIN>(gslab, a2g, dzg, params, step, B,
                                       nullptr, nullptr, MomArgs{});
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_reduce_update_mom(
    const float* __restrict__ gslab, const act_t* __restrict__ a2g,
    const float* __restrict__ dzg, float* __restrict__ params,
    float* __restrict__ vel, MomArgs o, int B) {
  reduce_update_body<act_t, OPT_MOM>(gslab, a2g, dzg, params, 0.f, B, vel,
                                     nullptr, o);
}

template <typename act_t>
__global__ __launch_bounds__(256) void k_reduce_update_adam(
    const float* __restrict__ gslab, const act_t* __restrict__ a2g,
    const float* __restrict__ dzg, float* __restrict__ params,
    float* __restrict__ vel, float* __restrict__ sq, AdamArgs o, int B) {
  reduce_update_body<act_t, OPT_ADAM>(gslab, a2g, dzg, params, 0.f, B, vel,
                                      sq, o);
}

}  // namespace pcnn

// ---------------------------------------------------------------------------
// extern "C" launchers, declared in ../pcnn_launch.h (called from the pybind
// layer and the native tools; no torch headers here).  All return hipError_t
// as int.  A launcher that applies the update takes the optimizer as a
// pcnn_opt: kind == 1 launches the _adam kernel; otherwise vel == NULL
// launches the plain kernel with opt->step, anything else the _mom kernel
// (opt_select, sgd_update.h).
// ---------------------------------------------------------------------------

// Loss scaling is a DeepCNN feature: this family's in-block step never
// stores a gradient in activation dtype.  Every launcher that takes an
// optimizer refuses a scaler state (pcnn_opt.ls_state) with this code.
enum { LS_REFUSED = -3 };

using namespace pcnn;

namespace {
template <int MODE>
int launch_fwdbwd_mode(const void* x, const float* params, void* a1, void* a2,
                       float* y, float* dz, float* dz2, void* dz1,
                       const int* labels, float* loss_accum, int* correct,
                       int B, int act, int pool_mode, int loss_mode,
                       float* grads, int wgrad_fuse, hipStream_t stream) {
  dim3 grid(B), block(256);
  PCNN_DISPATCH(act, hipLaunchKernelGGL(
                         (k_fwdbwd<act_t, MODE>), grid, block, 0, stream,
                         (const act_t*)x, params, (act_t*)a1, (act_t*)a2, y,
                         dz, dz2, (act_t*)dz1, labels, loss_accum, correct, B,
                         pool_mode, loss_mode, grads, wgrad_fuse));
  return (int)hipGetLastError();
}

// ticket == nullptr launches the plain k_wgrad; otherwise k_wgrad_update or
// k_wgrad_update_mom / k_wgrad_update_adam (by opt_select) with the same grid.
int launch_wgrad_any(const void* x, const void* a1, const void* a2,
                     const float* dz, const float* dz2, const void* dz1,
                     float* grads, int B, int act, int chunk_imgs, int roles,
                     float* params, const pcnn_opt* opt, int* ticket,
                     hipStream_t s) {
  // Batch-adaptive defaults: ~36 (image,position) items per conv thread,
  // pool slices at GC/4, fc batch slices of ~64 images.
  int GC = chunk_imgs > 0 ? chunk_imgs : (int)(4.0f * __builtin_cbrtf((float)B) + 0.5f);
  if (GC < 2) GC = 2;
  if (GC > 256) GC = 256;
  if (roles == 4) GC = 0;  // fc-only launch (fused-wgrad mode)
  // pool-role slices: ~10 (image,cell) items per thread (2 blocks at B=64
  // left the pool role as the kernel's longest pole)
  int GS = (B * S1_OUT + 256 * 5 - 1) / (256 * 5);
  if (GS < 2) GS = 2;
  if (GS > 96) GS = 96;
  if (roles == 4) GS = 0;
  int FS = B / 64;
  if (FS < 1) FS = 1;
  if (FS > 32) FS = 32;
  dim3 grid(C1_CH * GC + GS + FS * FC_BLOCKS), block(256);
  if (ticket != nullptr && opt->ls_state != nullptr) return LS_REFUSED;
  const int sel = ticket == nullptr ? OPT_PLAIN : opt_select(opt);
  if (sel < 0) return (int)hipErrorInvalidValue;
  PCNN_DISPATCH(act, {
    const act_t *xs = (const act_t*)x, *a1s = (const act_t*)a1,
                *a2s = (const act_t*)a2, *dz1s = (const act_t*)dz1;
    if (ticket == nullptr)
      hipLaunchKernelGGL((k_wgrad<act_t>), grid, block, 0, s, xs, a1s, a2s,
                         dz, dz2, dz1s, grads, B, GC, GS, FS, roles);
    else if (sel == OPT_ADAM)
      hipLaunchKernelGGL((k_wgrad_update_adam<act_t>), grid, block, 0, s, xs,
                         a1s, a2s, dz, dz2, dz1s, grads, B, GC, GS, FS, roles,
                         params, opt->vel, opt->sq, adam_args(opt), ticket);
    else if (sel == OPT_MOM)
      hipLaunchKernelGGL((k_wgrad_update_mom<act_t>), grid, block, 0, s, xs,
                         a1s, a2s, dz, dz2, dz1s, grads, B, GC, GS, FS, roles,
                         params, opt->vel, mom_args(opt), ticket);
    else
      hipLaunchKernelGGL((k_wgrad_update<act_t>), grid, block, 0, s, xs, a1s,
                         a2s, dz, dz2, dz1s, grads, B, GC, GS, FS, roles,
                         params, opt->step, ticket);
  });
  return (int)hipGetLastError();
}
}  // namespace

extern "C" {

int pcnn_launch_fwdbwd(const void* x, const float* params, void* a1, void* a2,
                       float* y, float* dz, float* dz2, void* dz1,
                       const int* labels, float* loss_accum, int* correct,
                       int B, int act, int mode, int pool_mode, int loss_mode,
                       float* grads, int wgrad_fuse, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (mode) {
    case MODE_TRAIN:
      return launch_fwdbwd_mode<MODE_TRAIN>(x, params, a1, a2, y, dz, dz2,
                                            dz1, labels, loss_accum, correct,
                                            B, act, pool_mode, loss_mode,
                                            grads, wgrad_fuse, s);
    case MODE_EVAL:
      return launch_fwdbwd_mode<MODE_EVAL>(x, params, a1, a2, y, dz, dz2, dz1,
                                           labels, loss_accum, correct, B,
                                           act, pool_mode, loss_mode, grads,
                                           wgrad_fuse, s);
    default:
      return launch_fwdbwd_mode<MODE_INFER>(x, params, a1, a2, y, dz, dz2,
                                            dz1, labels, loss_accum, correct,
                                            B, act, pool_mode, loss_mode,
                                            grads, wgrad_fuse, s);
  }
}

int pcnn_launch_wgrad(const void* x, const void* a1, const void* a2,
                      const float* dz, const float* dz2, const void* dz1,
                      float* grads, int B, int act, int chunk_imgs, int roles,
                      void* stream) {
  return launch_wgrad_any(x, a1, a2, dz, dz2, dz1, grads, B, act, chunk_imgs,
                          roles, nullptr, nullptr, nullptr,
                          (hipStream_t)stream);
}

int pcnn_launch_update(float* params, float* grads, const pcnn_opt* opt,
                       void* stream) {
  if (opt == nullptr) return (int)hipErrorInvalidValue;
  if (opt->ls_state != nullptr) return LS_REFUSED;
  dim3 grid((N_PARAMS / 4 + 255) / 256), block(256);
  const int sel = opt_select(opt);
  if (sel < 0) return (int)hipErrorInvalidValue;
  if (sel == OPT_ADAM)
    hipLaunchKernelGGL(k_update_adam, grid, block, 0, (hipStream_t)stream,
                       params, grads, opt->vel, opt->sq, adam_args(opt));
  else if (sel == OPT_MOM)
    hipLaunchKernelGGL(k_update_mom, grid, block, 0, (hipStream_t)stream,
                       params, grads, opt->vel, mom_args(opt));
  else
    hipLaunchKernelGGL(k_update, grid, block, 0, (hipStream_t)stream, params,
                       grads, opt->step);
  return (int)hipGetLastError();
}

// Weight gradients + update in one launch (k_wgrad_update[_mom|_adam]).
int pcnn_launch_wgrad_update(const void* x, const void* a1, const void* a2,
                             const float* dz, const float* dz2,
                             const void* dz1, float* grads, float* params,
                             const pcnn_opt* opt, int* ticket, int B, int act,
                             int chunk_imgs, int roles, void* stream) {
  if (ticket == nullptr || params == nullptr || opt == nullptr)
    return (int)hipErrorInvalidValue;
  // Measured crossover (MI355X, us/step, fused vs three launches in one
  // job): B=16 17.16 vs 17.37, 64 18.45 vs 18.96, 256 23.64 vs 23.88,
  // 1024 42.31 vs 42.43, 4096 bf16 101.2 vs 100.7, 4096 fp16 101.6 vs
  // 102.0.  The tail saves a fixed ~0.5 us at best; by B=4096 the
  // thousands of blocks that each drain and draw a ticket have used it up
  // and the difference is noise, so large batches keep the kernel boundary.
  if (B > 2048) {
    const int err = pcnn_launch_wgrad(x, a1, a2, dz, dz2, dz1, grads, B, act,
                                      chunk_imgs, roles, stream);
    if (err != 0) return err;
    return pcnn_launch_update(params, grads, opt, stream);
  }
  return launch_wgrad_any(x, a1, a2, dz, dz2, dz1, grads, B, act, chunk_imgs,
                          roles, params, opt, ticket, (hipStream_t)stream);
}

int pcnn_inblock_default_variant(void) { return INBLOCK_DEFAULT_VARIANT; }

// First kernel of the in-block weight-grad step in train mode.  Writes a2,
// y, dz, the loss sum and rows [0, B) of gslab ([>= B][GSLAB_LD] fp32); a1,
// dz1 and dz2 are not produced.  variant: 0 = cell (k_fwdbwd<.., INBLOCK>,
// one lane per pool cell, 256 threads), 1 = pair (k_fwdbwd_pair, two lanes
// per cell, 512 threads), -1 = INBLOCK_DEFAULT_VARIANT.
int pcnn_launch_fwdbwd_inblock(const void* x, const float* params, void* a2,
                               float* y, float* dz, const int* labels,
                               float* loss_accum, float* gslab, int B, int act,
                               int pool_mode, int loss_mode, int variant,
                               void* stream) {
  if (gslab == nullptr || dz == nullptr || B < 1 || variant < -1 ||
      variant > 1)
    return (int)hipErrorInvalidValue;
  if (variant < 0) variant = INBLOCK_DEFAULT_VARIANT;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(B);
  if (variant == 1) {
    PCNN_DISPATCH(act, hipLaunchKernelGGL(
                           (k_fwdbwd_pair<act_t>), grid, dim3(PR_THREADS), 0,
                           s, (const act_t*)x, params, (act_t*)a2, y, dz,
                           labels, loss_accum, B, pool_mode, loss_mode,
                           gslab));
  } else {
    PCNN_DISPATCH(act, hipLaunchKernelGGL(
                           (k_fwdbwd<act_t, MODE_TRAIN, true>), grid,
                           dim3(256), 0, s, (const act_t*)x, params,
                           (act_t*)nullptr, (act_t*)a2, y, dz,
                           (float*)nullptr, (act_t*)nullptr, labels,
                           loss_accum, (int*)nullptr, B, pool_mode, loss_mode,
                           gslab, 0));
  }
  return (int)hipGetLastError();
}

// Second kernel of the in-block weight-grad step
// (k_reduce_update[_mom|_adam]).
int pcnn_launch_reduce_update(const float* gslab, const void* a2,
                              const float* dz, float* params,
                              const pcnn_opt* opt, int B, int act,
                              void* stream) {
  if (gslab == nullptr || params == nullptr || opt == nullptr || B < 1)
    return (int)hipErrorInvalidValue;
  if (opt->ls_state != nullptr) return LS_REFUSED;
  dim3 grid(RU_BLOCKS), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int sel = opt_select(opt);
  if (sel < 0) return (int)hipErrorInvalidValue;
  if (sel == OPT_ADAM)
    PCNN_DISPATCH(act, hipLaunchKernelGGL(
                           (k_reduce_update_adam<act_t>), grid, block, 0, s,
                           gslab, (const act_t*)a2, dz, params, opt->vel,
                           opt->sq, adam_args(opt), B));
  else if (sel == OPT_MOM)
    PCNN_DISPATCH(act, hipLaunchKernelGGL(
                           (k_reduce_update_mom<act_t>), grid, block, 0, s,
                           gslab, (const act_t*)a2, dz, params, opt->vel,
                           mom_args(opt), B));
  else
    PCNN_DISPATCH(act, hipLaunchKernelGGL(
                           (k_reduce_update<act_t>), grid, block, 0, s, gslab,
                           (const act_t*)a2, dz, params, opt->step, B));
  return (int)hipGetLastError();
}

// Largest batch that runs the in-block weight-grad step; above it the step
// launcher below runs k_fwdbwd + k_wgrad_update as before.
int pcnn_inblock_max_batch(void) { return INBLOCK_MAX_B; }

// One whole single-GPU training step with in-block weight grads:
// k_fwdbwd<INBLOCK> or k_fwdbwd_pair -> k_reduce_update[_mom|_adam].  `grads`
// and `ticket` are only touched by the large-batch fallback and read
// all-zero / 0 afterwards either way.
int pcnn_launch_step_inblock(const void* x, float* params, void* a1, void* a2,
                             float* y, float* dz, float* dz2, void* dz1,
                             const int* labels, float* loss_accum,
                             float* grads, int* ticket, float* gslab,
                             const pcnn_opt* opt, int B, int act,
                             int pool_mode, int loss_mode, int chunk_imgs,
                             int variant, void* stream) {
  // refused before the forward/backward launch, not after it
  if (opt != nullptr && opt->ls_state != nullptr) return LS_REFUSED;
  // k_reduce_update walks the batch with 4 lanes per parameter, so its cost
  // grows linearly with B while k_wgrad_update spreads a larger batch over
  // more blocks.  Measured (MI355X, bf16, us/step, in-block vs
  // k_wgrad_update in one job, in-block at every size): B=16 12.33 vs
  // 17.08, 64 13.60 vs 18.60, 256 21.22 vs 23.64, 1024 54.08 vs 42.16,
  // 4096 175.9 vs 100.7 (profiles/r4).  256 is the last measured gain,
  // 1024 the first measured loss; nothing was measured in between, so the
  // true crossover lies somewhere in (256, 1024) and batches there keep the
  // k_wgrad_update step without having been compared.
  if (B > INBLOCK_MAX_B) {
    // Role mask as Trainer._wroles builds it: all roles, minus the pool
    // role under max pooling.  The fc-only mask (4) belongs to fuse_wgrad,
    // which excludes this step.
    int err = pcnn_launch_fwdbwd(x, params, a1, a2, y, dz, dz2, dz1, labels,
                                 loss_accum, nullptr, B, act, MODE_TRAIN,
                                 pool_mode, loss_mode, grads, 0, stream);
    if (err != 0) return err;
    return pcnn_launch_wgrad_update(x, a1, a2, dz, dz2, dz1, grads, params,
                                    opt, ticket, B, act, chunk_imgs,
                                    pool_mode == 1 ? 5 : 7, stream);
  }
  int err = pcnn_launch_fwdbwd_inblock(x, params, a2, y, dz, labels,
                                       loss_accum, gslab, B, act, pool_mode,
                                       loss_mode, variant, stream);
  if (err != 0) return err;
  return pcnn_launch_reduce_update(gslab, a2, dz, params, opt, B, act,
                                   stream);
}

#ifdef PCNN_LENET_STAMPS
// Diagnostic build only: side buffer of the phase stamps,
// [blocks][512][16] 64-bit words.
int pcnn_stamp_set_buffer(void* buf, int blocks) {
  unsigned long long* p = (unsigned long long*)buf;
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(pcnn::g_stamps), &p, sizeof(p));
  if (e != hipSuccess) return (int)e;
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(pcnn::g_stamp_blocks), &blocks,
                                sizeof(blocks));
}
#endif

const char* pcnn_hip_error_string(int err) {
  return hipGetErrorString((hipError_t)err);
}
}

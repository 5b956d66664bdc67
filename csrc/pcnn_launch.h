/* The C launcher surface of csrc/hip/lenet_kernels.hip and
 * csrc/hip/conv_kernels.hip, declared once.  Both .hip files include this
 * header, so every definition is checked against its declaration; every C or
 * C++ caller (csrc/bindings.cpp, tools/pcnn_train.cpp, tools/lt_probe.cpp)
 * includes it instead of writing prototypes of its own.  A ctypes caller has
 * no such check and must set argtypes from the signatures below.
 *
 * Plain C: no torch or HIP headers.  Streams cross as void* (a hipStream_t),
 * activation buffers as void* with the dtype flag `act` (0 = fp32, 1 = bf16,
 * 2 = fp16).  Every launcher returns a hipError_t as int (0 = success) or a
 * small negative number for a refused argument.
 */
#ifndef PCNN_LAUNCH_H
#define PCNN_LAUNCH_H

#ifdef __cplusplus
extern "C" {
#endif

/* The optimizer of every launcher that applies an update.
 * vel == NULL: plain SGD, p += step * g, with `step` = dt * scale multiplied
 * by the caller (the launchers never recompute it); the other fields are
 * ignored.  vel != NULL: the momentum kernels, u = scale*g - wd*p;
 * v = mu*v + u; p += dt*v (nesterov: p += dt*(u + mu*v)); `step` is ignored.
 * vel is the fp32 velocity bucket in the layout of params.
 *
 * kind == 1: the Adam kernels (decoupled weight decay), whatever vel says:
 * u = scale*g; m = beta1*m + (1-beta1)*u; s = beta2*s + (1-beta2)*u*u;
 * p += dt*((c1*m)/(c2*sqrt(s) + eps) - wd*p).  vel carries m, mu carries
 * beta1, sq is s (fp32, layout of params); both buckets are required.  The
 * caller computes per update, in double, c1 = 1/(1-beta1^t) and
 * c2 = 1/sqrt(1-beta2^t) for the 1-based update count t, and omb1 = 1-beta1,
 * omb2 = 1-beta2 (1.f - beta2 in float would carry beta2's own rounding).
 * `step` and `nesterov` are ignored.  The fields from `kind` on were
 * appended: an initialiser that stops at vel leaves them zero, kind 0.
 *
 * ls_state (appended last; NULL = everything above, unchanged): the loss
 * scaler's device state, PCNN_LS_WORDS 32-bit words laid out as float scale,
 * float inv_scale, int32 found_inf, int32 good_steps, int32 skipped, int32 t,
 * float c1, float c2.  The bucket then holds scale x the gradients.  With
 * found_inf set the update kernels zero the gradient bucket and touch
 * nothing else; with it clear they apply the update with `step` (plain) or
 * `scale` (momentum, Adam) multiplied by inv_scale, and Adam reads c1, c2
 * from the state instead of from this struct.  DeepCNN launchers only: the
 * LeNet launchers refuse a non-NULL ls_state with -3. */
#define PCNN_LS_WORDS 8
typedef struct pcnn_opt {
  float step;
  float scale, dt, mu, wd;
  int nesterov;
  float* vel;
  int kind;
  float* sq;
  float beta2, eps, c1, c2;
  float omb1, omb2;
  const float* ls_state;
} pcnn_opt;

const char* pcnn_hip_error_string(int err);

/* ---- LeNet step (lenet_kernels.hip) ---- */
/* mode: 0 = train, 1 = eval, 2 = infer */
int pcnn_launch_fwdbwd(const void* x, const float* params, void* a1, void* a2,
                       float* y, float* dz, float* dz2, void* dz1,
                       const int* labels, float* loss_accum, int* correct,
                       int B, int act, int mode, int pool_mode, int loss_mode,
                       float* grads, int wgrad_fuse, void* stream);
/* chunk_imgs: conv1 slices per channel, <= 0 = default; roles: bitmask
 * 1 = conv1, 2 = pool, 4 = fc */
int pcnn_launch_wgrad(const void* x, const void* a1, const void* a2,
                      const float* dz, const float* dz2, const void* dz1,
                      float* grads, int B, int act, int chunk_imgs, int roles,
                      void* stream);
int pcnn_launch_update(float* params, float* grads, const pcnn_opt* opt,
                       void* stream);
/* ticket: one device int32 that reads 0 before the launch and 0 after it */
int pcnn_launch_wgrad_update(const void* x, const void* a1, const void* a2,
                             const float* dz, const float* dz2,
                             const void* dz1, float* grads, float* params,
                             const pcnn_opt* opt, int* ticket, int B, int act,
                             int chunk_imgs, int roles, void* stream);
/* variant: 0 = cell kernel, 1 = pair kernel, -1 = the default */
int pcnn_inblock_default_variant(void);
int pcnn_inblock_max_batch(void);
int pcnn_launch_fwdbwd_inblock(const void* x, const float* params, void* a2,
                               float* y, float* dz, const int* labels,
                               float* loss_accum, float* gslab, int B, int act,
                               int pool_mode, int loss_mode, int variant,
                               void* stream);
int pcnn_launch_reduce_update(const float* gslab, const void* a2,
                              const float* dz, float* params,
                              const pcnn_opt* opt, int B, int act,
                              void* stream);
int pcnn_launch_step_inblock(const void* x, float* params, void* a1, void* a2,
                             float* y, float* dz, float* dz2, void* dz1,
                             const int* labels, float* loss_accum,
                             float* grads, int* ticket, float* gslab,
                             const pcnn_opt* opt, int B, int act,
                             int pool_mode, int loss_mode, int chunk_imgs,
                             int variant, void* stream);
/* -DPCNN_LENET_STAMPS builds only (tools/phase_stamps.py) */
int pcnn_stamp_set_buffer(void* buf, int blocks);

/* ---- DeepCNN (conv_kernels.hip) ---- */
int pcnn_deep_im2col(const void* x, void* cols, int B, int H, int W, int Cin,
                     int K, int P, int KcP, int act, void* stream);
int pcnn_deep_gemm(const void* A, const float* Bsrc, const void* Bpre,
                   const float* bias, void* C, long long M, int K, int N,
                   int ldA, int ldC, int b_kxn, int epilogue, const void* imx,
                   int XH, int XW, int XC, int XK, int XP, const void* epi,
                   const float* pw, void* pout, int PK, float* c32,
                   long long c32_cap, int act, void* stream);
int pcnn_deep_cast_wt(const float* W, void* out, void* outT, int R, int C,
                      void* stream);
/* The nine per-stage descriptor arrays of the batched weight cast, each
 * n_stages long; p8_off may be NULL (no 8-padded image). */
typedef struct pcnn_cast_desc {
  int n_stages;
  const int *R, *C, *K, *Cin;
  const long long *w_off, *bf_off, *bfT_off, *rot_off, *p8_off;
} pcnn_cast_desc;
int pcnn_deep_cast_all(const float* params, void* wbuf,
                       const pcnn_cast_desc* desc, void* stream);
int pcnn_deep_update_cast(float* params, float* grads, long long n,
                          const pcnn_opt* opt, void* wbuf,
                          const pcnn_cast_desc* desc, void* stream);
int pcnn_deep_update(float* params, float* grads, long long n,
                     const pcnn_opt* opt, void* stream);
int pcnn_deep_wgrad_gemm(const void* cols, const void* dpre, float* dW,
                         float* part, long long M, int KcP, int N, int MS,
                         const void* imx, int XH, int XW, int XC, int XK,
                         int XP, float* db, int act, void* stream);
int pcnn_deep_wgrad_multi(int n_stages, const void* const* a,
                          const void* const* dpre, float* const* dW,
                          float* const* db, const long long* M,
                          const int* KcP, const int* N, const int* MS,
                          const int* implicit, const int* XH, const int* XW,
                          const int* XC, const int* XK, const int* XP, int act,
                          void* stream);
int pcnn_deep_pad_channels(const void* x, void* x8, long long npix, int Cin,
                           int act, void* stream);
int pcnn_deep_remap_dw8(float* dW8, float* dW, int KK, int Cin, int Cout,
                        void* stream);
int pcnn_deep_colsum(const void* dpre, float* part, float* db, long long M,
                     int N, int slices, int act, void* stream);
int pcnn_deep_col2im_sigbwd(const void* dcols, const void* pout, void* out,
                            int B, int H, int W, int Cin, int K, int P,
                            int KcP, int act, void* stream);
int pcnn_deep_pool_fwd(const void* a, const float* pw, void* pout, int B,
                       int H, int W, int C, int K, int act, void* stream);
int pcnn_deep_pool_bwd(const void* dppre, const void* a, const float* pw,
                       void* dapre, int B, int H, int W, int C, int K, int act,
                       void* stream);
int pcnn_deep_pool_wgrad(const void* dppre, const void* a, float* dpw, int B,
                         int H, int W, int C, int K, int G, int act,
                         void* stream);
int pcnn_deep_pool_wbwd(const void* dppre, const void* a, const float* pw,
                        void* dapre, float* dpw, int B, int H, int W, int C,
                        int K, int G, int act, void* stream);
int pcnn_deep_fc_fwd(const void* flat, const float* fw, const float* fb,
                     const int* labels, float* yg, float* dzg,
                     float* loss_accum, int* correct_accum, int B, int FCIN,
                     int NCLS, int mode, void* dflat, const float* ls_state,
                     int act, void* stream);
int pcnn_deep_fc_bwd(const float* dzg, const void* flat, const float* fw,
                     void* dflat, int B, int FCIN, int NCLS, int act,
                     void* stream);
int pcnn_deep_fc_wgrad(const float* dzg, const void* flat, float* gfw,
                       float* gfb, int B, int FCIN, int NCLS, int FS, int act,
                       void* stream);
/* Loss scaling.  ls_check: one pass over the flat gradient bucket (16-byte
 * aligned); any inf or NaN sets found_inf, nothing ever clears it here.
 * ls_advance: one thread, after the update.  found_inf set: scale =
 * max(scale/2, 1), good_steps = 0, skipped += 1, t and c1, c2 stay.  Clear:
 * t += 1, c1 = 1/(1-beta1^t), c2 = 1/sqrt(1-beta2^t) in double, good_steps
 * += 1 and, on reaching growth_interval, scale = min(2*scale, 2^24) and
 * good_steps = 0.  dynamic == 0 (a fixed scale) leaves scale and good_steps
 * alone; skips are still counted.  found_inf is cleared at the end. */
int pcnn_deep_ls_check(const float* grads, long long n, float* ls_state,
                       void* stream);
int pcnn_deep_ls_advance(float* ls_state, int growth_interval, int dynamic,
                         double beta1, double beta2, void* stream);
int pcnn_deep_mfma_selftest(const float* A, const float* Bm, float* D,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCNN_LAUNCH_H */

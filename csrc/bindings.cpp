// pybind11 bindings for parallel_cnn_amd._C
//
// CPU ops take at::Tensor directly.  GPU launchers live in
// csrc/hip/*.hip (compiled by hipcc for gfx950, linked in as objects) and
// are declared in pcnn_launch.h, the only place their prototypes are
// written; this translation unit deliberately includes no HIP headers —
// streams cross the boundary as opaque pointers obtained from
// torch.cuda.current_stream().cuda_stream on the Python side.

#include <torch/extension.h>

#include <cmath>

#include "lenet_dims.h"
#include "pcnn_launch.h"

namespace pcnn {
void cpu_forward(at::Tensor x, at::Tensor params, at::Tensor a1, at::Tensor a2,
                 at::Tensor y, int64_t pool_mode, int64_t loss_mode);
double cpu_backward(at::Tensor x, at::Tensor params, at::Tensor a1,
                    at::Tensor a2, at::Tensor y, at::Tensor labels,
                    at::Tensor dz, at::Tensor dz2, at::Tensor dz1,
                    at::Tensor grads, int64_t pool_mode, int64_t loss_mode);
void cpu_update(at::Tensor params, at::Tensor grads, double dt, double scale);
void cpu_update_momentum(at::Tensor params, at::Tensor grads, at::Tensor vel,
                         double dt, double scale, double mu, double wd,
                         bool nesterov);
void cpu_update_adam(at::Tensor params, at::Tensor grads, at::Tensor m,
                     at::Tensor sq, double dt, double scale, double beta1,
                     double beta2, double eps, double wd, int64_t t);
}  // namespace pcnn

namespace {

void check_hip(int err, const char* what) {
  TORCH_CHECK(err == 0, "HIP error in ", what, ": ",
              pcnn_hip_error_string(err));
}

int act_flag(const at::Tensor& t) {
  if (t.scalar_type() == at::kBFloat16) return 1;
  if (t.scalar_type() == at::kHalf) return 2;
  TORCH_CHECK(t.scalar_type() == at::kFloat,
              "activation tensors must be bf16, fp16 or fp32");
  return 0;
}

// mode: 0 = train, 1 = eval (argmax + correct count), 2 = infer
void hip_fwdbwd(at::Tensor x, at::Tensor params, at::Tensor a1, at::Tensor a2,
                at::Tensor y, at::Tensor dz, at::Tensor dz2, at::Tensor dz1,
                at::Tensor labels, at::Tensor loss_accum,
                at::Tensor correct_accum, int64_t B, int64_t mode,
                int64_t stream, int64_t pool_mode, int64_t loss_mode,
                at::Tensor grads, int64_t wgrad_fuse) {
  TORCH_CHECK(x.is_cuda() && params.is_cuda(), "expected device tensors");
  TORCH_CHECK(labels.scalar_type() == at::kInt, "labels must be int32");
  TORCH_CHECK(!dz1.numel() || dz1.scalar_type() == x.scalar_type(),
              "dz1 must match the activation dtype");
  int f = act_flag(x);
  check_hip(pcnn_launch_fwdbwd(
                x.data_ptr(), params.data_ptr<float>(), a1.data_ptr(),
                a2.data_ptr(), y.numel() ? y.data_ptr<float>() : nullptr,
                dz.numel() ? dz.data_ptr<float>() : nullptr,
                dz2.numel() ? dz2.data_ptr<float>() : nullptr,
                dz1.numel() ? dz1.data_ptr() : nullptr,
                labels.data_ptr<int>(),
                loss_accum.numel() ? loss_accum.data_ptr<float>() : nullptr,
                correct_accum.numel() ? correct_accum.data_ptr<int>() : nullptr,
                (int)B, f, (int)mode, (int)pool_mode, (int)loss_mode,
                grads.numel() ? grads.data_ptr<float>() : nullptr,
                (int)wgrad_fuse, (void*)stream),
            "fwdbwd");
}

// roles bitmask (1=conv1, 2=pool, 4=fc) — ablation/diagnostics only.
void hip_wgrad_roles(at::Tensor x, at::Tensor a1, at::Tensor a2,
                     at::Tensor dz, at::Tensor dz2, at::Tensor dz1,
                     at::Tensor grads, int64_t B, int64_t chunk_imgs,
                     int64_t roles, int64_t stream) {
  int f = act_flag(x);
  check_hip(pcnn_launch_wgrad(x.data_ptr(), a1.data_ptr(), a2.data_ptr(),
                              dz.data_ptr<float>(), dz2.data_ptr<float>(),
                              dz1.data_ptr(), grads.data_ptr<float>(), (int)B,
                              f, (int)chunk_imgs, (int)roles, (void*)stream),
            "wgrad_roles");
}

void hip_wgrad(at::Tensor x, at::Tensor a1, at::Tensor a2, at::Tensor dz,
               at::Tensor dz2, at::Tensor dz1, at::Tensor grads, int64_t B,
               int64_t chunk_imgs, int64_t stream) {
  TORCH_CHECK(dz1.scalar_type() == x.scalar_type(),
              "dz1 must match the activation dtype");
  check_hip(pcnn_launch_wgrad(x.data_ptr(), a1.data_ptr(), a2.data_ptr(),
                              dz.data_ptr<float>(), dz2.data_ptr<float>(),
                              dz1.data_ptr(), grads.data_ptr<float>(), (int)B,
                              act_flag(x), (int)chunk_imgs, 7, (void*)stream),
            "wgrad");
}

int* ticket_ptr(const at::Tensor& ticket) {
  TORCH_CHECK(ticket.is_cuda() && ticket.scalar_type() == at::kInt &&
                  ticket.numel() >= 1,
              "ticket must be a device int32 tensor");
  return ticket.data_ptr<int>();
}

// Velocity bucket of the momentum update.
float* vel_ptr(const at::Tensor& vel, const at::Tensor& params) {
  TORCH_CHECK(vel.is_cuda() && vel.scalar_type() == at::kFloat &&
                  vel.is_contiguous() && vel.numel() == params.numel(),
              "vel must be a contiguous device fp32 tensor with the same "
              "numel as params");
  return vel.data_ptr<float>();
}

// Second-moment bucket of the Adam update.
float* sq_ptr(const at::Tensor& sq, const at::Tensor& params) {
  TORCH_CHECK(sq.is_cuda() && sq.scalar_type() == at::kFloat &&
                  sq.is_contiguous() && sq.numel() == params.numel(),
              "sq must be a contiguous device fp32 tensor with the same "
              "numel as params");
  return sq.data_ptr<float>();
}

// Loss-scaler state (pcnn_opt.ls_state): PCNN_LS_WORDS device fp32 words, or
// None / an empty tensor for no loss scaling.
const float* ls_ptr(const c10::optional<at::Tensor>& ls) {
  if (!ls.has_value() || ls->numel() == 0) return nullptr;
  TORCH_CHECK(ls->is_cuda() && ls->scalar_type() == at::kFloat &&
                  ls->is_contiguous() && ls->numel() == PCNN_LS_WORDS,
              "ls_state must be a contiguous device fp32 tensor of ",
              PCNN_LS_WORDS, " words");
  return ls->data_ptr<float>();
}

// The optimizer of a launch (pcnn_opt, pcnn_launch.h): the plain bindings
// pass the pre-multiplied step and no velocity, which selects the plain
// kernels; the _momentum bindings pass dt and scale apart and the velocity
// bucket; the _adam bindings pass both moment buckets and the 1-based update
// count t, from which the bias corrections are formed here in double.
pcnn_opt plain_opt(double step) {
  return pcnn_opt{(float)step, 0.f, 0.f, 0.f, 0.f, 0, nullptr};
}

pcnn_opt momentum_opt(const at::Tensor& vel, const at::Tensor& params,
                      double dt, double scale, double mu, double wd,
                      bool nesterov) {
  return pcnn_opt{0.f,       (float)scale,     (float)dt,           (float)mu,
                  (float)wd, nesterov ? 1 : 0, vel_ptr(vel, params)};
}

pcnn_opt adam_opt(const at::Tensor& m, const at::Tensor& sq,
                  const at::Tensor& params, double dt, double scale,
                  double beta1, double beta2, double eps, double wd,
                  int64_t t) {
  TORCH_CHECK(t >= 1, "t is the 1-based update count");
  pcnn_opt o = {};
  o.scale = (float)scale;
  o.dt = (float)dt;
  o.mu = (float)beta1;
  o.wd = (float)wd;
  o.vel = vel_ptr(m, params);
  o.kind = 1;
  o.sq = sq_ptr(sq, params);
  o.beta2 = (float)beta2;
  o.eps = (float)eps;
  o.c1 = (float)(1.0 / (1.0 - std::pow(beta1, (double)t)));
  o.c2 = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)t)));
  o.omb1 = (float)(1.0 - beta1);
  o.omb2 = (float)(1.0 - beta2);
  return o;
}

void check_flat_buckets(const at::Tensor& params, const at::Tensor& grads) {
  TORCH_CHECK(params.is_cuda() && grads.is_cuda() &&
                  params.numel() == pcnn::N_PARAMS &&
                  grads.numel() == pcnn::N_PARAMS,
              "params/grads must be the flat device buckets");
}

void hip_update(at::Tensor params, at::Tensor grads, double step,
                int64_t stream) {
  const pcnn_opt opt = plain_opt(step);
  check_hip(pcnn_launch_update(params.data_ptr<float>(),
                               grads.data_ptr<float>(), &opt, (void*)stream),
            "update");
}

// hip_update with momentum / Nesterov / weight decay (k_update_mom).
void hip_update_momentum(at::Tensor params, at::Tensor grads, at::Tensor vel,
                         double dt, double scale, double mu, double wd,
                         bool nesterov, int64_t stream) {
  check_flat_buckets(params, grads);
  const pcnn_opt opt = momentum_opt(vel, params, dt, scale, mu, wd, nesterov);
  check_hip(pcnn_launch_update(params.data_ptr<float>(),
                               grads.data_ptr<float>(), &opt, (void*)stream),
            "update_momentum");
}

// hip_update with the Adam rule (k_update_adam).
void hip_update_adam(at::Tensor params, at::Tensor grads, at::Tensor m,
                     at::Tensor sq, double dt, double scale, double beta1,
                     double beta2, double eps, double wd, int64_t t,
                     int64_t stream) {
  check_flat_buckets(params, grads);
  const pcnn_opt opt =
      adam_opt(m, sq, params, dt, scale, beta1, beta2, eps, wd, t);
  check_hip(pcnn_launch_update(params.data_ptr<float>(),
                               grads.data_ptr<float>(), &opt, (void*)stream),
            "update_adam");
}

// Weight gradients with the SGD update as the tail of the same launch:
// the last block to arrive on `ticket` applies the update and zeroes g.
void wgrad_update_impl(const at::Tensor& x, const at::Tensor& a1,
                       const at::Tensor& a2, const at::Tensor& dz,
                       const at::Tensor& dz2, const at::Tensor& dz1,
                       const at::Tensor& grads, const at::Tensor& params,
                       const pcnn_opt& opt, const at::Tensor& ticket,
                       int64_t B, int64_t chunk_imgs, int64_t roles,
                       int64_t stream, const char* what) {
  int f = act_flag(x);
  TORCH_CHECK(dz1.scalar_type() == x.scalar_type(),
              "dz1 must match the activation dtype");
  check_flat_buckets(params, grads);
  check_hip(pcnn_launch_wgrad_update(
                x.data_ptr(), a1.data_ptr(), a2.data_ptr(),
                dz.data_ptr<float>(), dz2.data_ptr<float>(), dz1.data_ptr(),
                grads.data_ptr<float>(), params.data_ptr<float>(), &opt,
                ticket_ptr(ticket), (int)B, f, (int)chunk_imgs, (int)roles,
                (void*)stream),
            what);
}

void hip_wgrad_update(at::Tensor x, at::Tensor a1, at::Tensor a2,
                      at::Tensor dz, at::Tensor dz2, at::Tensor dz1,
                      at::Tensor grads, at::Tensor params, double step,
                      at::Tensor ticket, int64_t B, int64_t chunk_imgs,
                      int64_t roles, int64_t stream) {
  wgrad_update_impl(x, a1, a2, dz, dz2, dz1, grads, params, plain_opt(step),
                    ticket, B, chunk_imgs, roles, stream, "wgrad_update");
}

// hip_wgrad_update with the momentum tail (k_wgrad_update_mom).
void hip_wgrad_update_momentum(at::Tensor x, at::Tensor a1, at::Tensor a2,
                               at::Tensor dz, at::Tensor dz2, at::Tensor dz1,
                               at::Tensor grads, at::Tensor params,
                               at::Tensor vel, double dt, double scale,
                               double mu, double wd, bool nesterov,
                               at::Tensor ticket, int64_t B,
                               int64_t chunk_imgs, int64_t roles,
                               int64_t stream) {
  wgrad_update_impl(x, a1, a2, dz, dz2, dz1, grads, params,
                    momentum_opt(vel, params, dt, scale, mu, wd, nesterov),
                    ticket, B, chunk_imgs, roles, stream,
                    "wgrad_update_momentum");
}

// hip_wgrad_update with the Adam tail (k_wgrad_update_adam).
void hip_wgrad_update_adam(at::Tensor x, at::Tensor a1, at::Tensor a2,
                           at::Tensor dz, at::Tensor dz2, at::Tensor dz1,
                           at::Tensor grads, at::Tensor params, at::Tensor m,
                           at::Tensor sq, double dt, double scale,
                           double beta1, double beta2, double eps, double wd,
                           int64_t t, at::Tensor ticket, int64_t B,
                           int64_t chunk_imgs, int64_t roles,
                           int64_t stream) {
  wgrad_update_impl(
      x, a1, a2, dz, dz2, dz1, grads, params,
      adam_opt(m, sq, params, dt, scale, beta1, beta2, eps, wd, t), ticket, B,
      chunk_imgs, roles, stream, "wgrad_update_adam");
}

float* gslab_ptr(const at::Tensor& gslab, int64_t B) {
  TORCH_CHECK(gslab.is_cuda() && gslab.scalar_type() == at::kFloat &&
                  gslab.is_contiguous() &&
                  gslab.numel() >= B * pcnn::GSLAB_LD,
              "gslab must be a contiguous device fp32 [>=B, ",
              pcnn::GSLAB_LD, "] tensor");
  return gslab.data_ptr<float>();
}

// Kernel 1 of the in-block step: 0 = cell (k_fwdbwd<.., INBLOCK>), 1 = pair
// (k_fwdbwd_pair), -1 = the library default (_C.INBLOCK_DEFAULT_VARIANT).
int inblock_variant(int64_t variant) {
  TORCH_CHECK(variant >= -1 && variant <= 1,
              "variant must be -1 (default), 0 (cell) or 1 (pair)");
  return (int)variant;
}

// First kernel of the in-block weight-grad step on its own: forward +
// backward-data in train mode, with this batch's conv/pool gradient sums
// written to rows [0, B) of gslab.  a1, dz1 and dz2 are not produced.
void hip_fwdbwd_inblock(at::Tensor x, at::Tensor params, at::Tensor a2,
                        at::Tensor y, at::Tensor dz, at::Tensor labels,
                        at::Tensor loss_accum, at::Tensor gslab, int64_t B,
                        int64_t stream, int64_t pool_mode,
                        int64_t loss_mode, int64_t variant) {
  TORCH_CHECK(x.is_cuda() && params.is_cuda(), "expected device tensors");
  TORCH_CHECK(labels.scalar_type() == at::kInt, "labels must be int32");
  TORCH_CHECK(B >= 1 && x.numel() >= B * pcnn::IN_PIX &&
                  a2.numel() >= B * pcnn::S1_OUT &&
                  a2.scalar_type() == x.scalar_type() &&
                  y.numel() >= B * pcnn::FC_OUT &&
                  dz.numel() >= B * pcnn::FC_OUT && labels.numel() >= B,
              "buffers too small for B");
  check_hip(pcnn_launch_fwdbwd_inblock(
                x.data_ptr(), params.data_ptr<float>(), a2.data_ptr(),
                y.data_ptr<float>(), dz.data_ptr<float>(),
                labels.data_ptr<int>(),
                loss_accum.numel() ? loss_accum.data_ptr<float>() : nullptr,
                gslab_ptr(gslab, B), (int)B, act_flag(x), (int)pool_mode,
                (int)loss_mode, inblock_variant(variant), (void*)stream),
            "fwdbwd_inblock");
}

// One whole training step with in-block weight grads (k_fwdbwd<INBLOCK> or
// k_fwdbwd_pair -> k_reduce_update[_mom|_adam]); above
// _C.INBLOCK_MAX_BATCH the launcher runs k_fwdbwd ->
// k_wgrad_update[_mom|_adam] instead, which is why it takes every buffer.
void step_inblock_impl(const at::Tensor& x, const at::Tensor& params,
                       const at::Tensor& a1, const at::Tensor& a2,
                       const at::Tensor& y, const at::Tensor& dz,
                       const at::Tensor& dz2, const at::Tensor& dz1,
                       const at::Tensor& labels, const at::Tensor& loss_accum,
                       const at::Tensor& grads, const at::Tensor& ticket,
                       const at::Tensor& gslab, const pcnn_opt& opt,
                       int64_t B, int64_t chunk_imgs, int64_t stream,
                       int64_t pool_mode, int64_t loss_mode, int64_t variant,
                       const char* what) {
  TORCH_CHECK(x.is_cuda() && params.is_cuda(), "expected device tensors");
  TORCH_CHECK(labels.scalar_type() == at::kInt, "labels must be int32");
  TORCH_CHECK(dz1.scalar_type() == x.scalar_type() &&
                  a2.scalar_type() == x.scalar_type(),
              "a2/dz1 must match the activation dtype");
  TORCH_CHECK(params.numel() == pcnn::N_PARAMS &&
                  grads.numel() == pcnn::N_PARAMS,
              "params/grads must be the flat device buckets");
  TORCH_CHECK(B >= 1 && x.numel() >= B * pcnn::IN_PIX &&
                  a2.numel() >= B * pcnn::S1_OUT &&
                  y.numel() >= B * pcnn::FC_OUT &&
                  dz.numel() >= B * pcnn::FC_OUT && labels.numel() >= B,
              "buffers too small for B");
  TORCH_CHECK(B <= pcnn_inblock_max_batch() ||
                  (a1.numel() >= B * pcnn::C1_OUT &&
                   dz1.numel() >= B * pcnn::C1_OUT &&
                   dz2.numel() >= B * pcnn::S1_OUT),
              "a1/dz1/dz2 too small for the large-batch path");
  check_hip(pcnn_launch_step_inblock(
                x.data_ptr(), params.data_ptr<float>(), a1.data_ptr(),
                a2.data_ptr(), y.data_ptr<float>(), dz.data_ptr<float>(),
                dz2.data_ptr<float>(), dz1.data_ptr(), labels.data_ptr<int>(),
                loss_accum.data_ptr<float>(), grads.data_ptr<float>(),
                ticket_ptr(ticket), gslab_ptr(gslab, B), &opt, (int)B,
                act_flag(x), (int)pool_mode, (int)loss_mode, (int)chunk_imgs,
                inblock_variant(variant), (void*)stream),
            what);
}

void hip_step_inblock(at::Tensor x, at::Tensor params, at::Tensor a1,
                      at::Tensor a2, at::Tensor y, at::Tensor dz,
                      at::Tensor dz2, at::Tensor dz1, at::Tensor labels,
                      at::Tensor loss_accum, at::Tensor grads,
                      at::Tensor ticket, at::Tensor gslab, double step,
                      int64_t B, int64_t chunk_imgs, int64_t stream,
                      int64_t pool_mode, int64_t loss_mode,
                      int64_t variant) {
  step_inblock_impl(x, params, a1, a2, y, dz, dz2, dz1, labels, loss_accum,
                    grads, ticket, gslab, plain_opt(step), B, chunk_imgs,
                    stream, pool_mode, loss_mode, variant, "step_inblock");
}

void hip_step_inblock_momentum(at::Tensor x, at::Tensor params,
                               at::Tensor vel, at::Tensor a1, at::Tensor a2,
                               at::Tensor y, at::Tensor dz, at::Tensor dz2,
                               at::Tensor dz1, at::Tensor labels,
                               at::Tensor loss_accum, at::Tensor grads,
                               at::Tensor ticket, at::Tensor gslab, double dt,
                               double scale, double mu, double wd,
                               bool nesterov, int64_t B, int64_t chunk_imgs,
                               int64_t stream, int64_t pool_mode,
                               int64_t loss_mode, int64_t variant) {
  step_inblock_impl(x, params, a1, a2, y, dz, dz2, dz1, labels, loss_accum,
                    grads, ticket, gslab,
                    momentum_opt(vel, params, dt, scale, mu, wd, nesterov), B,
                    chunk_imgs, stream, pool_mode, loss_mode, variant,
                    "step_inblock_momentum");
}

void hip_step_inblock_adam(at::Tensor x, at::Tensor params, at::Tensor m,
                           at::Tensor sq, at::Tensor a1, at::Tensor a2,
                           at::Tensor y, at::Tensor dz, at::Tensor dz2,
                           at::Tensor dz1, at::Tensor labels,
                           at::Tensor loss_accum, at::Tensor grads,
                           at::Tensor ticket, at::Tensor gslab, double dt,
                           double scale, double beta1, double beta2,
                           double eps, double wd, int64_t t, int64_t B,
                           int64_t chunk_imgs, int64_t stream,
                           int64_t pool_mode, int64_t loss_mode,
                           int64_t variant) {
  step_inblock_impl(
      x, params, a1, a2, y, dz, dz2, dz1, labels, loss_accum, grads, ticket,
      gslab, adam_opt(m, sq, params, dt, scale, beta1, beta2, eps, wd, t), B,
      chunk_imgs, stream, pool_mode, loss_mode, variant, "step_inblock_adam");
}

// Second kernel of the in-block step on its own: slab rows [0, B), a2 and dz
// in, params and the optimizer state updated.
void reduce_update_impl(const at::Tensor& gslab, const at::Tensor& a2,
                        const at::Tensor& dz, const at::Tensor& params,
                        const pcnn_opt& opt, int64_t B, int64_t stream,
                        const char* what) {
  TORCH_CHECK(params.is_cuda() && params.numel() == pcnn::N_PARAMS,
              "params must be the flat device bucket");
  TORCH_CHECK(B >= 1 && a2.is_cuda() && a2.numel() >= B * pcnn::S1_OUT &&
                  dz.is_cuda() && dz.scalar_type() == at::kFloat &&
                  dz.numel() >= B * pcnn::FC_OUT,
              "buffers too small for B");
  check_hip(pcnn_launch_reduce_update(gslab_ptr(gslab, B), a2.data_ptr(),
                                      dz.data_ptr<float>(),
                                      params.data_ptr<float>(), &opt, (int)B,
                                      act_flag(a2), (void*)stream),
            what);
}

// Plain form (k_reduce_update): params += step * g.
void hip_reduce_update(at::Tensor gslab, at::Tensor a2, at::Tensor dz,
                       at::Tensor params, double step, int64_t B,
                       int64_t stream) {
  reduce_update_impl(gslab, a2, dz, params, plain_opt(step), B, stream,
                     "reduce_update");
}

// Momentum form (k_reduce_update_mom).
void hip_reduce_update_momentum(at::Tensor gslab, at::Tensor a2,
                                at::Tensor dz, at::Tensor params,
                                at::Tensor vel, double dt, double scale,
                                double mu, double wd, bool nesterov,
                                int64_t B, int64_t stream) {
  reduce_update_impl(gslab, a2, dz, params,
                     momentum_opt(vel, params, dt, scale, mu, wd, nesterov),
                     B, stream, "reduce_update_momentum");
}

// Adam form (k_reduce_update_adam).
void hip_reduce_update_adam(at::Tensor gslab, at::Tensor a2, at::Tensor dz,
                            at::Tensor params, at::Tensor m, at::Tensor sq,
                            double dt, double scale, double beta1,
                            double beta2, double eps, double wd, int64_t t,
                            int64_t B, int64_t stream) {
  reduce_update_impl(
      gslab, a2, dz, params,
      adam_opt(m, sq, params, dt, scale, beta1, beta2, eps, wd, t), B, stream,
      "reduce_update_adam");
}

// Single-GPU fused training loop: enqueues `steps` full training steps
// from C++, cycling a device-resident batch pool.  step_mode 3 is
// fwd+bwd-data -> wgrad -> update; step_mode 2 is fwd+bwd-data ->
// wgrad+update (needs `ticket`); step_mode 4 is the in-block weight-grad
// step, fwd+bwd-data+conv/pool grads -> reduce+update (needs `ticket` and
// `gslab`).  Asynchronous — caller syncs the stream.
// The distributed path keeps the per-step Python loop (the all-reduce sits
// between wgrad and update there).
void hip_train_steps(at::Tensor x_pool, at::Tensor labels_pool,
                     at::Tensor params, at::Tensor grads, at::Tensor a1,
                     at::Tensor a2, at::Tensor y, at::Tensor dz,
                     at::Tensor dz2, at::Tensor dz1, at::Tensor loss_accum,
                     int64_t B, int64_t steps, int64_t chunk_imgs,
                     double step_scale, int64_t stream, int64_t pool_mode,
                     int64_t loss_mode, int64_t wgrad_fuse,
                     int64_t step_mode, at::Tensor ticket,
                     at::Tensor gslab, at::Tensor vel, double dt,
                     double scale, double mu, double wd, bool nesterov,
                     int64_t variant, at::Tensor sq, double beta2, double eps,
                     int64_t t0) {
  const int var = inblock_variant(variant);
  // a non-empty vel selects the momentum update in every step mode; dt and
  // scale then replace the pre-multiplied step_scale.  A non-empty sq
  // selects Adam instead: vel is then m, mu is beta1, t0 is the number of
  // updates already applied, and the bias corrections are formed again for
  // t = t0 + st + 1 at every step of the loop below.
  const bool adam = sq.numel() != 0;
  TORCH_CHECK(!adam || t0 >= 0, "t0 is the number of updates applied so far");
  pcnn_opt opt =
      adam ? adam_opt(vel, sq, params, dt, scale, mu, beta2, eps, wd, t0 + 1)
      : vel.numel() ? momentum_opt(vel, params, dt, scale, mu, wd, nesterov)
                    : plain_opt(step_scale);
  TORCH_CHECK(step_mode == 3 || step_mode == 2 || step_mode == 4,
              "step_mode must be 3, 2 or 4");
  TORCH_CHECK(step_mode == 3 || !wgrad_fuse,
              "the two-launch steps exclude wgrad_fuse");
  int* tk = step_mode != 3 ? ticket_ptr(ticket) : nullptr;
  float* slab = step_mode == 4 ? gslab_ptr(gslab, B) : nullptr;
  // wgrad_fuse=1: conv/pool grads accumulate inside the fwdbwd kernel and
  // kernel B covers only the fc role.  Measured slower at bs=64 (the LDS
  // atomic combine serializes) — default off.
  const int wroles = wgrad_fuse ? 4 : (pool_mode == 1 ? 5 : 7);
  TORCH_CHECK(x_pool.is_cuda() && x_pool.dim() == 2, "x_pool [P*B, 784]");
  TORCH_CHECK(labels_pool.scalar_type() == at::kInt, "labels must be int32");
  const int64_t pool_rows = x_pool.size(0);
  TORCH_CHECK(pool_rows % B == 0, "pool rows must be a multiple of B");
  const int64_t P = pool_rows / B;
  const int f = act_flag(x_pool);
  const size_t esz = f ? 2 : 4;  // bf16/fp16 vs fp32
  const char* xp = (const char*)x_pool.data_ptr();
  const int* lp = labels_pool.data_ptr<int>();
  float* pp = params.data_ptr<float>();
  float* gp = grads.data_ptr<float>();
  void* s = (void*)stream;
  for (int64_t st = 0; st < steps; ++st) {
    const int64_t i = st % P;
    const void* xb = xp + (size_t)i * B * pcnn::IN_PIX * esz;
    const int* lb = lp + i * B;
    if (adam && st > 0)
      opt = adam_opt(vel, sq, params, dt, scale, mu, beta2, eps, wd,
                     t0 + st + 1);
    if (step_mode == 4) {
      check_hip(pcnn_launch_step_inblock(
                    xb, pp, a1.data_ptr(), a2.data_ptr(), y.data_ptr<float>(),
                    dz.data_ptr<float>(), dz2.data_ptr<float>(),
                    dz1.data_ptr(), lb, loss_accum.data_ptr<float>(), gp, tk,
                    slab, &opt, (int)B, f, (int)pool_mode, (int)loss_mode,
                    (int)chunk_imgs, var, s),
                "train_steps/step_inblock");
      continue;
    }
    check_hip(pcnn_launch_fwdbwd(xb, pp, a1.data_ptr(), a2.data_ptr(),
                                 y.data_ptr<float>(), dz.data_ptr<float>(),
                                 dz2.data_ptr<float>(), dz1.data_ptr(), lb,
                                 loss_accum.data_ptr<float>(), nullptr,
                                 (int)B, f, 0, (int)pool_mode, (int)loss_mode,
                                 gp, (int)wgrad_fuse, s),
              "train_steps/fwdbwd");
    if (step_mode == 2) {
      check_hip(pcnn_launch_wgrad_update(
                    xb, a1.data_ptr(), a2.data_ptr(), dz.data_ptr<float>(),
                    dz2.data_ptr<float>(), dz1.data_ptr(), gp, pp, &opt, tk,
                    (int)B, f, (int)chunk_imgs, wroles, s),
                "train_steps/wgrad_update");
      continue;
    }
    check_hip(pcnn_launch_wgrad(xb, a1.data_ptr(), a2.data_ptr(),
                                dz.data_ptr<float>(), dz2.data_ptr<float>(),
                                dz1.data_ptr(), gp, (int)B, f,
                                (int)chunk_imgs, wroles, s),
              "train_steps/wgrad");
    check_hip(pcnn_launch_update(pp, gp, &opt, s), "train_steps/update");
  }
}

// ---------------------------------------------------------------------------
// DeepCNN (general conv path) wrappers
// ---------------------------------------------------------------------------
void deep_im2col(at::Tensor x, at::Tensor cols, int64_t B, int64_t H,
                 int64_t W, int64_t Cin, int64_t K, int64_t P, int64_t KcP,
                 int64_t stream) {
  check_hip(pcnn_deep_im2col(x.data_ptr(), cols.data_ptr(), (int)B, (int)H,
                             (int)W, (int)Cin, (int)K, (int)P, (int)KcP,
                             act_flag(x), (void*)stream),
            "deep_im2col");
}

void deep_gemm(at::Tensor A, at::Tensor Bsrc, at::Tensor bias, at::Tensor C,
               int64_t M, int64_t K, int64_t N, int64_t ldA, int64_t ldC,
               int64_t b_kxn, int64_t epilogue, int64_t stream,
               at::Tensor Bpre, at::Tensor imx, int64_t XH, int64_t XW,
               int64_t XC, int64_t XK, int64_t XP, at::Tensor epi,
               at::Tensor pw, at::Tensor pout, int64_t PK, at::Tensor c32) {
  check_hip(pcnn_deep_gemm(
                A.data_ptr(), Bsrc.data_ptr<float>(),
                Bpre.numel() ? Bpre.data_ptr() : nullptr,
                bias.numel() ? bias.data_ptr<float>() : nullptr,
                C.data_ptr(), M, (int)K, (int)N, (int)ldA, (int)ldC,
                (int)b_kxn, (int)epilogue,
                imx.numel() ? imx.data_ptr() : nullptr, (int)XH, (int)XW,
                (int)XC, (int)XK, (int)XP,
                epi.numel() ? epi.data_ptr() : nullptr,
                pw.numel() ? pw.data_ptr<float>() : nullptr,
                pout.numel() ? pout.data_ptr() : nullptr, (int)PK,
                c32.numel() ? c32.data_ptr<float>() : nullptr,
                (long long)c32.numel(), act_flag(A), (void*)stream),
            "deep_gemm");
}

void deep_cast_wt(at::Tensor W, at::Tensor out, at::Tensor outT, int64_t R,
                  int64_t C, int64_t stream) {
  check_hip(pcnn_deep_cast_wt(W.data_ptr<float>(), out.data_ptr(),
                              outT.data_ptr(), (int)R, (int)C,
                              (void*)stream),
            "deep_cast_wt");
}

// The per-stage descriptor lists of the batched weight cast as the launchers
// take them (pcnn_cast_desc points into this object).
struct CastDesc {
  int R[8], C[8], K[8], Cin[8];
  long long w_off[8], bf_off[8], bfT_off[8], rot_off[8], p8_off[8];
  pcnn_cast_desc d;

  CastDesc(const char* what, const std::vector<int64_t>& Rv,
           const std::vector<int64_t>& Cv, const std::vector<int64_t>& Kv,
           const std::vector<int64_t>& Cinv, const std::vector<int64_t>& w,
           const std::vector<int64_t>& bf, const std::vector<int64_t>& bfT,
           const std::vector<int64_t>& rot, const std::vector<int64_t>& p8) {
    const size_t n = Rv.size();
    TORCH_CHECK(n >= 1 && n <= 8, what, ": 1..8 stages");
    TORCH_CHECK(Cv.size() == n && Kv.size() == n && Cinv.size() == n &&
                    w.size() == n && bf.size() == n && bfT.size() == n &&
                    rot.size() == n && (p8.empty() || p8.size() == n),
                what, ": descriptor length mismatch");
    for (size_t s = 0; s < n; ++s) {
      R[s] = (int)Rv[s];
      C[s] = (int)Cv[s];
      K[s] = (int)Kv[s];
      Cin[s] = (int)Cinv[s];
      w_off[s] = w[s];
      bf_off[s] = bf[s];
      bfT_off[s] = bfT[s];
      rot_off[s] = rot[s];
      p8_off[s] = p8.empty() ? -1 : p8[s];
    }
    d = pcnn_cast_desc{(int)n,  R,       C,      K,      Cin,
                       w_off,   bf_off,  bfT_off, rot_off, p8_off};
  }
  CastDesc(const CastDesc&) = delete;
};

void deep_cast_all(at::Tensor params, at::Tensor wbuf,
                   std::vector<int64_t> R, std::vector<int64_t> C,
                   std::vector<int64_t> K, std::vector<int64_t> Cin,
                   std::vector<int64_t> w_off, std::vector<int64_t> bf_off,
                   std::vector<int64_t> bfT_off,
                   std::vector<int64_t> rot_off,
                   std::vector<int64_t> p8_off, int64_t stream) {
  const CastDesc cd("deep_cast_all", R, C, K, Cin, w_off, bf_off, bfT_off,
                    rot_off, p8_off);
  check_hip(pcnn_deep_cast_all(params.data_ptr<float>(), wbuf.data_ptr(),
                               &cd.d, (void*)stream),
            "deep_cast_all");
}

void deep_update_cast(at::Tensor params, at::Tensor grads, double step,
                      at::Tensor wbuf, std::vector<int64_t> R,
                      std::vector<int64_t> C, std::vector<int64_t> K,
                      std::vector<int64_t> Cin, std::vector<int64_t> w_off,
                      std::vector<int64_t> bf_off,
                      std::vector<int64_t> bfT_off,
                      std::vector<int64_t> rot_off,
                      std::vector<int64_t> p8_off, int64_t stream,
    c10::optional<at::Tensor> ls_state) {
  const CastDesc cd("deep_update_cast", R, C, K, Cin, w_off, bf_off, bfT_off,
                    rot_off, p8_off);
  pcnn_opt opt = plain_opt(step);
  opt.ls_state = ls_ptr(ls_state);
  check_hip(pcnn_deep_update_cast(params.data_ptr<float>(),
                                  grads.data_ptr<float>(), params.numel(),
                                  &opt, wbuf.data_ptr(), &cd.d,
                                  (void*)stream),
            "deep_update_cast");
}

// deep_update_cast with momentum / Nesterov / weight decay: the bf16 images
// are cast from the post-momentum value.
void deep_update_cast_momentum(at::Tensor params, at::Tensor grads,
                               at::Tensor vel, double dt, double scale,
                               double mu, double wd, bool nesterov,
                               at::Tensor wbuf, std::vector<int64_t> R,
                               std::vector<int64_t> C, std::vector<int64_t> K,
                               std::vector<int64_t> Cin,
                               std::vector<int64_t> w_off,
                               std::vector<int64_t> bf_off,
                               std::vector<int64_t> bfT_off,
                               std::vector<int64_t> rot_off,
                               std::vector<int64_t> p8_off, int64_t stream,
    c10::optional<at::Tensor> ls_state) {
  const CastDesc cd("deep_update_cast_momentum", R, C, K, Cin, w_off, bf_off,
                    bfT_off, rot_off, p8_off);
  TORCH_CHECK(grads.numel() == params.numel(), "grads/params size mismatch");
  pcnn_opt opt = momentum_opt(vel, params, dt, scale, mu, wd, nesterov);
  opt.ls_state = ls_ptr(ls_state);
  check_hip(pcnn_deep_update_cast(params.data_ptr<float>(),
                                  grads.data_ptr<float>(), params.numel(),
                                  &opt, wbuf.data_ptr(), &cd.d,
                                  (void*)stream),
            "deep_update_cast_momentum");
}

// deep_update_cast with the Adam update (k_update_cast_all_adam): the bf16
// images are cast from the post-Adam value.
void deep_update_cast_adam(at::Tensor params, at::Tensor grads, at::Tensor m,
                           at::Tensor sq, double dt, double scale,
                           double beta1, double beta2, double eps, double wd,
                           int64_t t, at::Tensor wbuf, std::vector<int64_t> R,
                           std::vector<int64_t> C, std::vector<int64_t> K,
                           std::vector<int64_t> Cin,
                           std::vector<int64_t> w_off,
                           std::vector<int64_t> bf_off,
                           std::vector<int64_t> bfT_off,
                           std::vector<int64_t> rot_off,
                           std::vector<int64_t> p8_off, int64_t stream,
    c10::optional<at::Tensor> ls_state) {
  const CastDesc cd("deep_update_cast_adam", R, C, K, Cin, w_off, bf_off,
                    bfT_off, rot_off, p8_off);
  TORCH_CHECK(grads.numel() == params.numel(), "grads/params size mismatch");
  pcnn_opt opt = adam_opt(m, sq, params, dt, scale, beta1, beta2, eps, wd, t);
  opt.ls_state = ls_ptr(ls_state);
  check_hip(pcnn_deep_update_cast(params.data_ptr<float>(),
                                  grads.data_ptr<float>(), params.numel(),
                                  &opt, wbuf.data_ptr(), &cd.d,
                                  (void*)stream),
            "deep_update_cast_adam");
}

void deep_wgrad_multi(std::vector<at::Tensor> a,
                      std::vector<at::Tensor> dpre,
                      std::vector<at::Tensor> dW, std::vector<at::Tensor> db,
                      std::vector<int64_t> M, std::vector<int64_t> KcP,
                      std::vector<int64_t> N, std::vector<int64_t> MS,
                      std::vector<int64_t> implicit, std::vector<int64_t> XH,
                      std::vector<int64_t> XW, std::vector<int64_t> XC,
                      std::vector<int64_t> XK, std::vector<int64_t> XP,
                      int64_t stream) {
  const size_t n = a.size();
  TORCH_CHECK(n >= 1 && n <= 8, "deep_wgrad_multi: 1..8 stages");
  const void* ap[8];
  const void* dp[8];
  float* wp[8];
  float* bp[8];
  long long Mi[8];
  int Ki[8], Ni[8], MSi[8], Ii[8], XHi[8], XWi[8], XCi[8], XKi[8], XPi[8];
  for (size_t s = 0; s < n; ++s) {
    ap[s] = a[s].data_ptr();
    dp[s] = dpre[s].data_ptr();
    wp[s] = dW[s].data_ptr<float>();
    bp[s] = db[s].data_ptr<float>();
    Mi[s] = M[s];
    Ki[s] = (int)KcP[s];
    Ni[s] = (int)N[s];
    MSi[s] = (int)MS[s];
    Ii[s] = (int)implicit[s];
    XHi[s] = (int)XH[s];
    XWi[s] = (int)XW[s];
    XCi[s] = (int)XC[s];
    XKi[s] = (int)XK[s];
    XPi[s] = (int)XP[s];
  }
  check_hip(pcnn_deep_wgrad_multi((int)n, ap, dp, wp, bp, Mi, Ki, Ni, MSi,
                                  Ii, XHi, XWi, XCi, XKi, XPi,
                                  act_flag(dpre[0]), (void*)stream),
            "deep_wgrad_multi");
}

void deep_pad_channels(at::Tensor x, at::Tensor x8, int64_t npix,
                       int64_t Cin, int64_t stream) {
  check_hip(pcnn_deep_pad_channels(x.data_ptr(), x8.data_ptr(), npix,
                                   (int)Cin, act_flag(x), (void*)stream),
            "deep_pad_channels");
}

void deep_remap_dw8(at::Tensor dW8, at::Tensor dW, int64_t KK, int64_t Cin,
                    int64_t Cout, int64_t stream) {
  check_hip(pcnn_deep_remap_dw8(dW8.data_ptr<float>(), dW.data_ptr<float>(),
                                (int)KK, (int)Cin, (int)Cout,
                                (void*)stream),
            "deep_remap_dw8");
}

void deep_wgrad_gemm(at::Tensor cols, at::Tensor dpre, at::Tensor dW,
                     int64_t M, int64_t KcP, int64_t N, int64_t MS,
                     int64_t stream, at::Tensor imx, int64_t XH, int64_t XW,
                     int64_t XC, int64_t XK, int64_t XP, at::Tensor part,
                     at::Tensor db) {
  float* pp = nullptr;
  if (part.numel()) {
    TORCH_CHECK(part.numel() >= MS * KcP * N, "wgrad slab scratch too small");
    pp = part.data_ptr<float>();
  }
  check_hip(pcnn_deep_wgrad_gemm(
                cols.data_ptr(), dpre.data_ptr(), dW.data_ptr<float>(), pp, M,
                (int)KcP, (int)N, (int)MS,
                imx.numel() ? imx.data_ptr() : nullptr, (int)XH, (int)XW,
                (int)XC, (int)XK, (int)XP,
                db.numel() ? db.data_ptr<float>() : nullptr,
                act_flag(cols), (void*)stream),
            "deep_wgrad_gemm");
}

void deep_colsum(at::Tensor dpre, at::Tensor part, at::Tensor db, int64_t M,
                 int64_t N, int64_t slices, int64_t stream) {
  TORCH_CHECK(part.numel() >= slices * N, "colsum scratch too small");
  check_hip(pcnn_deep_colsum(dpre.data_ptr(), part.data_ptr<float>(),
                             db.data_ptr<float>(), M, (int)N, (int)slices,
                             act_flag(dpre), (void*)stream),
            "deep_colsum");
}

void deep_col2im_sigbwd(at::Tensor dcols, at::Tensor pout, at::Tensor out,
                        int64_t B, int64_t H, int64_t W, int64_t Cin,
                        int64_t K, int64_t P, int64_t KcP, int64_t stream) {
  check_hip(pcnn_deep_col2im_sigbwd(
                dcols.data_ptr(), pout.numel() ? pout.data_ptr() : nullptr,
                out.data_ptr(), (int)B, (int)H, (int)W, (int)Cin, (int)K,
                (int)P, (int)KcP, act_flag(dcols), (void*)stream),
            "deep_col2im_sigbwd");
}

void deep_pool_fwd(at::Tensor a, at::Tensor pw, at::Tensor pout, int64_t B,
                   int64_t H, int64_t W, int64_t C, int64_t K,
                   int64_t stream) {
  check_hip(pcnn_deep_pool_fwd(a.data_ptr(), pw.data_ptr<float>(),
                               pout.data_ptr(), (int)B, (int)H, (int)W,
                               (int)C, (int)K, act_flag(a), (void*)stream),
            "deep_pool_fwd");
}

void deep_pool_bwd(at::Tensor dppre, at::Tensor a, at::Tensor pw,
                   at::Tensor dapre, int64_t B, int64_t H, int64_t W,
                   int64_t C, int64_t K, int64_t stream) {
  check_hip(pcnn_deep_pool_bwd(dppre.data_ptr(), a.data_ptr(),
                               pw.data_ptr<float>(), dapre.data_ptr(),
                               (int)B, (int)H, (int)W, (int)C, (int)K,
                               act_flag(a), (void*)stream),
            "deep_pool_bwd");
}

void deep_pool_wgrad(at::Tensor dppre, at::Tensor a, at::Tensor dpw,
                     int64_t B, int64_t H, int64_t W, int64_t C, int64_t K,
                     int64_t G, int64_t stream) {
  check_hip(pcnn_deep_pool_wgrad(dppre.data_ptr(), a.data_ptr(),
                                 dpw.data_ptr<float>(), (int)B, (int)H,
                                 (int)W, (int)C, (int)K, (int)G,
                                 act_flag(a), (void*)stream),
            "deep_pool_wgrad");
}

void deep_pool_wbwd(at::Tensor dppre, at::Tensor a, at::Tensor pw,
                    at::Tensor dapre, at::Tensor dpw, int64_t B, int64_t H,
                    int64_t W, int64_t C, int64_t K, int64_t G,
                    int64_t stream) {
  check_hip(pcnn_deep_pool_wbwd(dppre.data_ptr(), a.data_ptr(),
                                pw.data_ptr<float>(), dapre.data_ptr(),
                                dpw.data_ptr<float>(), (int)B, (int)H,
                                (int)W, (int)C, (int)K, (int)G,
                                act_flag(a), (void*)stream),
            "deep_pool_wbwd");
}

void deep_fc_fwd(at::Tensor flat, at::Tensor fw, at::Tensor fb,
                 at::Tensor labels, at::Tensor y, at::Tensor dz,
                 at::Tensor loss_accum, at::Tensor correct_accum, int64_t B,
                 int64_t FCIN, int64_t NCLS, int64_t mode, int64_t stream,
                 at::Tensor dflat, c10::optional<at::Tensor> ls_state) {
  check_hip(pcnn_deep_fc_fwd(
                flat.data_ptr(), fw.data_ptr<float>(), fb.data_ptr<float>(),
                labels.data_ptr<int>(),
                y.numel() ? y.data_ptr<float>() : nullptr,
                dz.numel() ? dz.data_ptr<float>() : nullptr,
                loss_accum.numel() ? loss_accum.data_ptr<float>() : nullptr,
                correct_accum.numel() ? correct_accum.data_ptr<int>()
                                      : nullptr,
                (int)B, (int)FCIN, (int)NCLS, (int)mode,
                dflat.numel() ? dflat.data_ptr() : nullptr, ls_ptr(ls_state),
                act_flag(flat), (void*)stream),
            "deep_fc_fwd");
}

void deep_fc_bwd(at::Tensor dz, at::Tensor flat, at::Tensor fw,
                 at::Tensor dflat, int64_t B, int64_t FCIN, int64_t NCLS,
                 int64_t stream) {
  check_hip(pcnn_deep_fc_bwd(dz.data_ptr<float>(), flat.data_ptr(),
                             fw.data_ptr<float>(), dflat.data_ptr(), (int)B,
                             (int)FCIN, (int)NCLS, act_flag(flat),
                             (void*)stream),
            "deep_fc_bwd");
}

void deep_fc_wgrad(at::Tensor dz, at::Tensor flat, at::Tensor gfw,
                   at::Tensor gfb, int64_t B, int64_t FCIN, int64_t NCLS,
                   int64_t FS, int64_t stream) {
  check_hip(pcnn_deep_fc_wgrad(dz.data_ptr<float>(), flat.data_ptr(),
                               gfw.data_ptr<float>(), gfb.data_ptr<float>(),
                               (int)B, (int)FCIN, (int)NCLS, (int)FS,
                               act_flag(flat), (void*)stream),
            "deep_fc_wgrad");
}

void deep_update(at::Tensor params, at::Tensor grads, double step,
                 int64_t stream, c10::optional<at::Tensor> ls_state) {
  pcnn_opt opt = plain_opt(step);
  opt.ls_state = ls_ptr(ls_state);
  check_hip(pcnn_deep_update(params.data_ptr<float>(),
                             grads.data_ptr<float>(), params.numel(), &opt,
                             (void*)stream),
            "deep_update");
}

void deep_update_momentum(at::Tensor params, at::Tensor grads,
                          at::Tensor vel, double dt, double scale, double mu,
                          double wd, bool nesterov, int64_t stream,
                          c10::optional<at::Tensor> ls_state) {
  TORCH_CHECK(grads.numel() == params.numel(), "grads/params size mismatch");
  pcnn_opt opt = momentum_opt(vel, params, dt, scale, mu, wd, nesterov);
  opt.ls_state = ls_ptr(ls_state);
  check_hip(pcnn_deep_update(params.data_ptr<float>(),
                             grads.data_ptr<float>(), params.numel(), &opt,
                             (void*)stream),
            "deep_update_momentum");
}

void deep_update_adam(at::Tensor params, at::Tensor grads, at::Tensor m,
                      at::Tensor sq, double dt, double scale, double beta1,
                      double beta2, double eps, double wd, int64_t t,
                      int64_t stream, c10::optional<at::Tensor> ls_state) {
  TORCH_CHECK(grads.numel() == params.numel(), "grads/params size mismatch");
  pcnn_opt opt = adam_opt(m, sq, params, dt, scale, beta1, beta2, eps, wd, t);
  opt.ls_state = ls_ptr(ls_state);
  check_hip(pcnn_deep_update(params.data_ptr<float>(),
                             grads.data_ptr<float>(), params.numel(), &opt,
                             (void*)stream),
            "deep_update_adam");
}

// Overflow check of a flat fp32 gradient bucket into the scaler state.
void deep_ls_check(at::Tensor grads, at::Tensor ls_state, int64_t stream) {
  TORCH_CHECK(grads.is_cuda() && grads.scalar_type() == at::kFloat &&
                  grads.is_contiguous() && grads.numel() >= 1,
              "grads must be a contiguous device fp32 tensor");
  check_hip(pcnn_deep_ls_check(grads.data_ptr<float>(), grads.numel(),
                               const_cast<float*>(ls_ptr(ls_state)),
                               (void*)stream),
            "deep_ls_check");
}

// The scaler's step after an update (k_ls_advance).
void deep_ls_advance(at::Tensor ls_state, int64_t growth_interval,
                     bool dynamic, double beta1, double beta2,
                     int64_t stream) {
  check_hip(pcnn_deep_ls_advance(const_cast<float*>(ls_ptr(ls_state)),
                                 (int)growth_interval, dynamic ? 1 : 0, beta1,
                                 beta2, (void*)stream),
            "deep_ls_advance");
}

// Scaler state from host values: found_inf starts clear, inv_scale is formed
// here.  c1, c2 belong to update t (tools/deep_emul.py: adam_corrections).
void deep_ls_init(at::Tensor ls_state, double scale, int64_t good_steps,
                  int64_t skipped, int64_t t, double c1, double c2) {
  TORCH_CHECK(ls_ptr(ls_state) != nullptr, "ls_state must not be empty");
  TORCH_CHECK(scale >= 1.0 && t >= 1 && good_steps >= 0 && skipped >= 0,
              "deep_ls_init: scale >= 1, t >= 1, counters >= 0");
  at::Tensor host = at::empty({PCNN_LS_WORDS}, at::kFloat);
  float* f = host.data_ptr<float>();
  int32_t* w = reinterpret_cast<int32_t*>(f);
  f[0] = (float)scale;
  f[1] = 1.0f / (float)scale;
  w[2] = 0;
  w[3] = (int32_t)good_steps;
  w[4] = (int32_t)skipped;
  w[5] = (int32_t)t;
  f[6] = (float)c1;
  f[7] = (float)c2;
  ls_state.copy_(host);
}

// (scale, inv_scale, found_inf, good_steps, skipped, t, c1, c2); waits for
// the device like any .item().
py::tuple deep_ls_read(at::Tensor ls_state) {
  TORCH_CHECK(ls_ptr(ls_state) != nullptr, "ls_state must not be empty");
  at::Tensor host = ls_state.cpu().contiguous();
  const float* f = host.data_ptr<float>();
  const int32_t* w = reinterpret_cast<const int32_t*>(f);
  return py::make_tuple((double)f[0], (double)f[1], (int)w[2], (int)w[3],
                        (int)w[4], (int)w[5], (double)f[6], (double)f[7]);
}

void deep_mfma_selftest(at::Tensor A, at::Tensor Bm, at::Tensor D,
                        int64_t stream) {
  check_hip(pcnn_deep_mfma_selftest(A.data_ptr<float>(),
                                    Bm.data_ptr<float>(),
                                    D.data_ptr<float>(), (void*)stream),
            "deep_mfma_selftest");
}


}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "parallel_cnn_amd native ops (CPU reference + gfx950 HIP kernels)";
  m.def("cpu_forward", &pcnn::cpu_forward, py::arg("x"), py::arg("params"),
        py::arg("a1"), py::arg("a2"), py::arg("y"), py::arg("pool_mode") = 0,
        py::arg("loss_mode") = 0);
  m.def("cpu_backward", &pcnn::cpu_backward, py::arg("x"), py::arg("params"),
        py::arg("a1"), py::arg("a2"), py::arg("y"), py::arg("labels"),
        py::arg("dz"), py::arg("dz2"), py::arg("dz1"), py::arg("grads"),
        py::arg("pool_mode") = 0, py::arg("loss_mode") = 0);
  m.def("cpu_update", &pcnn::cpu_update);
  m.def("cpu_update_momentum", &pcnn::cpu_update_momentum, py::arg("params"),
        py::arg("grads"), py::arg("vel"), py::arg("dt"), py::arg("scale"),
        py::arg("mu"), py::arg("wd"), py::arg("nesterov"));
  m.def("cpu_update_adam", &pcnn::cpu_update_adam, py::arg("params"),
        py::arg("grads"), py::arg("m"), py::arg("sq"), py::arg("dt"),
        py::arg("scale"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("t"));
  m.def("hip_fwdbwd", &hip_fwdbwd, py::arg("x"), py::arg("params"),
        py::arg("a1"), py::arg("a2"), py::arg("y"), py::arg("dz"),
        py::arg("dz2"), py::arg("dz1"), py::arg("labels"),
        py::arg("loss_accum"), py::arg("correct_accum"), py::arg("B"),
        py::arg("mode"), py::arg("stream"), py::arg("pool_mode") = 0,
        py::arg("loss_mode") = 0, py::arg("grads") = at::empty({0}),
        py::arg("wgrad_fuse") = 0);
  m.def("hip_wgrad", &hip_wgrad);
  m.def("hip_wgrad_roles", &hip_wgrad_roles);
  m.def("hip_update", &hip_update);
  m.def("hip_train_steps", &hip_train_steps, py::arg("x_pool"),
        py::arg("labels_pool"), py::arg("params"), py::arg("grads"),
        py::arg("a1"), py::arg("a2"), py::arg("y"), py::arg("dz"),
        py::arg("dz2"), py::arg("dz1"), py::arg("loss_accum"), py::arg("B"),
        py::arg("steps"), py::arg("chunk_imgs"), py::arg("step_scale"),
        py::arg("stream"), py::arg("pool_mode") = 0,
        py::arg("loss_mode") = 0, py::arg("wgrad_fuse") = 0,
        py::arg("step_mode") = 3, py::arg("ticket") = at::empty({0}),
        py::arg("gslab") = at::empty({0}), py::arg("vel") = at::empty({0}),
        py::arg("dt") = 0.0, py::arg("scale") = 1.0, py::arg("mu") = 0.0,
        py::arg("wd") = 0.0, py::arg("nesterov") = false,
        py::arg("variant") = -1, py::arg("sq") = at::empty({0}),
        py::arg("beta2") = 0.999, py::arg("eps") = 1e-8, py::arg("t0") = 0);
  m.def("hip_update_adam", &hip_update_adam, py::arg("params"),
        py::arg("grads"), py::arg("m"), py::arg("sq"), py::arg("dt"),
        py::arg("scale"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("t"), py::arg("stream"));
  m.def("hip_wgrad_update_adam", &hip_wgrad_update_adam, py::arg("x"),
        py::arg("a1"), py::arg("a2"), py::arg("dz"), py::arg("dz2"),
        py::arg("dz1"), py::arg("grads"), py::arg("params"), py::arg("m"),
        py::arg("sq"), py::arg("dt"), py::arg("scale"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("t"),
        py::arg("ticket"), py::arg("B"), py::arg("chunk_imgs"),
        py::arg("roles"), py::arg("stream"));
  m.def("hip_reduce_update_adam", &hip_reduce_update_adam, py::arg("gslab"),
        py::arg("a2"), py::arg("dz"), py::arg("params"), py::arg("m"),
        py::arg("sq"), py::arg("dt"), py::arg("scale"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("t"),
        py::arg("B"), py::arg("stream"));
  m.def("hip_step_inblock_adam", &hip_step_inblock_adam, py::arg("x"),
        py::arg("params"), py::arg("m"), py::arg("sq"), py::arg("a1"),
        py::arg("a2"), py::arg("y"), py::arg("dz"), py::arg("dz2"),
        py::arg("dz1"), py::arg("labels"), py::arg("loss_accum"),
        py::arg("grads"), py::arg("ticket"), py::arg("gslab"), py::arg("dt"),
        py::arg("scale"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("t"), py::arg("B"), py::arg("chunk_imgs"),
        py::arg("stream"), py::arg("pool_mode") = 0,
        py::arg("loss_mode") = 0, py::arg("variant") = -1);
  m.def("hip_update_momentum", &hip_update_momentum, py::arg("params"),
        py::arg("grads"), py::arg("vel"), py::arg("dt"), py::arg("scale"),
        py::arg("mu"), py::arg("wd"), py::arg("nesterov"),
        py::arg("stream"));
  m.def("hip_wgrad_update_momentum", &hip_wgrad_update_momentum,
        py::arg("x"), py::arg("a1"), py::arg("a2"), py::arg("dz"),
        py::arg("dz2"), py::arg("dz1"), py::arg("grads"), py::arg("params"),
        py::arg("vel"), py::arg("dt"), py::arg("scale"), py::arg("mu"),
        py::arg("wd"), py::arg("nesterov"), py::arg("ticket"), py::arg("B"),
        py::arg("chunk_imgs"), py::arg("roles"), py::arg("stream"));
  m.def("hip_reduce_update", &hip_reduce_update, py::arg("gslab"),
        py::arg("a2"), py::arg("dz"), py::arg("params"), py::arg("step"),
        py::arg("B"), py::arg("stream"));
  m.def("hip_reduce_update_momentum", &hip_reduce_update_momentum,
        py::arg("gslab"), py::arg("a2"), py::arg("dz"), py::arg("params"),
        py::arg("vel"), py::arg("dt"), py::arg("scale"), py::arg("mu"),
        py::arg("wd"), py::arg("nesterov"), py::arg("B"), py::arg("stream"));
  m.def("hip_step_inblock_momentum", &hip_step_inblock_momentum,
        py::arg("x"), py::arg("params"), py::arg("vel"), py::arg("a1"),
        py::arg("a2"), py::arg("y"), py::arg("dz"), py::arg("dz2"),
        py::arg("dz1"), py::arg("labels"), py::arg("loss_accum"),
        py::arg("grads"), py::arg("ticket"), py::arg("gslab"), py::arg("dt"),
        py::arg("scale"), py::arg("mu"), py::arg("wd"), py::arg("nesterov"),
        py::arg("B"), py::arg("chunk_imgs"), py::arg("stream"),
        py::arg("pool_mode") = 0, py::arg("loss_mode") = 0,
        py::arg("variant") = -1);
  m.def("hip_fwdbwd_inblock", &hip_fwdbwd_inblock, py::arg("x"),
        py::arg("params"), py::arg("a2"), py::arg("y"), py::arg("dz"),
        py::arg("labels"), py::arg("loss_accum"), py::arg("gslab"),
        py::arg("B"), py::arg("stream"), py::arg("pool_mode") = 0,
        py::arg("loss_mode") = 0, py::arg("variant") = -1);
  m.def("hip_step_inblock", &hip_step_inblock, py::arg("x"),
        py::arg("params"), py::arg("a1"), py::arg("a2"), py::arg("y"),
        py::arg("dz"), py::arg("dz2"), py::arg("dz1"), py::arg("labels"),
        py::arg("loss_accum"), py::arg("grads"), py::arg("ticket"),
        py::arg("gslab"), py::arg("step"), py::arg("B"),
        py::arg("chunk_imgs"), py::arg("stream"), py::arg("pool_mode") = 0,
        py::arg("loss_mode") = 0, py::arg("variant") = -1);
  m.def("hip_wgrad_update", &hip_wgrad_update, py::arg("x"), py::arg("a1"),
        py::arg("a2"), py::arg("dz"), py::arg("dz2"), py::arg("dz1"),
        py::arg("grads"), py::arg("params"), py::arg("step"),
        py::arg("ticket"), py::arg("B"), py::arg("chunk_imgs"),
        py::arg("roles"), py::arg("stream"));
  m.def("deep_im2col", &deep_im2col);
  m.def("deep_gemm", &deep_gemm, py::arg("A"), py::arg("Bsrc"),
        py::arg("bias"), py::arg("C"), py::arg("M"), py::arg("K"),
        py::arg("N"), py::arg("ldA"), py::arg("ldC"), py::arg("b_kxn"),
        py::arg("epilogue"), py::arg("stream"),
        py::arg("Bpre") = at::empty({0}),
        py::arg("imx") = at::empty({0}), py::arg("XH") = 0,
        py::arg("XW") = 0, py::arg("XC") = 0, py::arg("XK") = 0,
        py::arg("XP") = 0, py::arg("epi") = at::empty({0}),
        py::arg("pw") = at::empty({0}), py::arg("pout") = at::empty({0}),
        py::arg("PK") = 0, py::arg("c32") = at::empty({0}));
  m.def("deep_cast_wt", &deep_cast_wt);
  m.def("deep_cast_all", &deep_cast_all);
  m.def("deep_pad_channels", &deep_pad_channels);
  m.def("deep_update_cast", &deep_update_cast, py::arg("params"),
        py::arg("grads"), py::arg("step"), py::arg("wbuf"), py::arg("R"), py::arg("C"), py::arg("K"),
        py::arg("Cin"), py::arg("w_off"), py::arg("bf_off"),
        py::arg("bfT_off"), py::arg("rot_off"), py::arg("p8_off"),
        py::arg("stream"), py::arg("ls_state") = py::none());
  m.def("deep_wgrad_multi", &deep_wgrad_multi);
  m.def("deep_remap_dw8", &deep_remap_dw8);
  m.def("deep_wgrad_gemm", &deep_wgrad_gemm, py::arg("cols"),
        py::arg("dpre"), py::arg("dW"), py::arg("M"), py::arg("KcP"),
        py::arg("N"), py::arg("MS"), py::arg("stream"),
        py::arg("imx") = at::empty({0}), py::arg("XH") = 0,
        py::arg("XW") = 0, py::arg("XC") = 0, py::arg("XK") = 0,
        py::arg("XP") = 0, py::arg("part") = at::empty({0}),
        py::arg("db") = at::empty({0}));
  m.def("deep_colsum", &deep_colsum);
  m.def("deep_col2im_sigbwd", &deep_col2im_sigbwd);
  m.def("deep_pool_fwd", &deep_pool_fwd);
  m.def("deep_pool_bwd", &deep_pool_bwd);
  m.def("deep_pool_wgrad", &deep_pool_wgrad);
  m.def("deep_pool_wbwd", &deep_pool_wbwd);
  m.def("deep_fc_fwd", &deep_fc_fwd, py::arg("flat"), py::arg("fw"),
        py::arg("fb"), py::arg("labels"), py::arg("y"), py::arg("dz"),
        py::arg("loss_accum"), py::arg("correct_accum"), py::arg("B"),
        py::arg("FCIN"), py::arg("NCLS"), py::arg("mode"),
        py::arg("stream"), py::arg("dflat") = at::empty({0}),
        py::arg("ls_state") = py::none());
  m.def("deep_fc_bwd", &deep_fc_bwd);
  m.def("deep_fc_wgrad", &deep_fc_wgrad);
  m.def("deep_update", &deep_update, py::arg("params"), py::arg("grads"),
        py::arg("step"), py::arg("stream"),
        py::arg("ls_state") = py::none());
  m.def("deep_update_momentum", &deep_update_momentum, py::arg("params"),
        py::arg("grads"), py::arg("vel"), py::arg("dt"), py::arg("scale"),
        py::arg("mu"), py::arg("wd"), py::arg("nesterov"), py::arg("stream"),
        py::arg("ls_state") = py::none());
  m.def("deep_update_cast_momentum", &deep_update_cast_momentum,
        py::arg("params"), py::arg("grads"), py::arg("vel"), py::arg("dt"),
        py::arg("scale"), py::arg("mu"), py::arg("wd"), py::arg("nesterov"),
        py::arg("wbuf"), py::arg("R"), py::arg("C"), py::arg("K"),
        py::arg("Cin"), py::arg("w_off"), py::arg("bf_off"),
        py::arg("bfT_off"), py::arg("rot_off"), py::arg("p8_off"),
        py::arg("stream"), py::arg("ls_state") = py::none());
  m.def("deep_update_adam", &deep_update_adam, py::arg("params"),
        py::arg("grads"), py::arg("m"), py::arg("sq"), py::arg("dt"),
        py::arg("scale"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("t"), py::arg("stream"),
        py::arg("ls_state") = py::none());
  m.def("deep_update_cast_adam", &deep_update_cast_adam, py::arg("params"),
        py::arg("grads"), py::arg("m"), py::arg("sq"), py::arg("dt"),
        py::arg("scale"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wd"), py::arg("t"), py::arg("wbuf"), py::arg("R"), py::arg("C"), py::arg("K"),
        py::arg("Cin"), py::arg("w_off"), py::arg("bf_off"),
        py::arg("bfT_off"), py::arg("rot_off"), py::arg("p8_off"),
        py::arg("stream"), py::arg("ls_state") = py::none());
  m.def("deep_ls_check", &deep_ls_check);
  m.def("deep_ls_advance", &deep_ls_advance);
  m.def("deep_ls_init", &deep_ls_init);
  m.def("deep_ls_read", &deep_ls_read);
  m.attr("LS_WORDS") = PCNN_LS_WORDS;
  m.def("deep_mfma_selftest", &deep_mfma_selftest);
  m.attr("N_PARAMS") = pcnn::N_PARAMS;
  m.attr("GSLAB_LD") = pcnn::GSLAB_LD;
  m.attr("INBLOCK_MAX_BATCH") = pcnn_inblock_max_batch();
  m.attr("INBLOCK_DEFAULT_VARIANT") = pcnn_inblock_default_variant();
  m.attr("OFF_C1W") = pcnn::OFF_C1W;
  m.attr("OFF_C1B") = pcnn::OFF_C1B;
  m.attr("OFF_S1W") = pcnn::OFF_S1W;
  m.attr("OFF_S1B") = pcnn::OFF_S1B;
  m.attr("OFF_FW") = pcnn::OFF_FW;
  m.attr("OFF_FB") = pcnn::OFF_FB;
  m.attr("REF_DT") = pcnn::REF_DT;
  m.attr("REF_THRESHOLD") = pcnn::REF_THRESHOLD;
  m.attr("HAS_HIP_KERNELS") = true;
}

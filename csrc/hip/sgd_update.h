// The update rule of every update kernel, device side.
//
// Included INSIDE the namespace of each .hip file (pcnn, pcnn_deep), after
// pcnn_launch.h: MomArgs and AdamArgs are kernel arguments, so their
// namespace is part of the kernels' symbol names, which profiles and tools
// refer to.
//
// Plain (OPT_PLAIN):  p += step*g
// Momentum / Nesterov / weight decay (OPT_MOM; ascent convention, g as the
// plain form reads it):
//   u = scale*g - wd*p;  v = mu*v + u;  p += dt*v
//   nesterov:            p += dt*(u + mu*v)     (v the freshly updated one)
// Adam with decoupled weight decay (OPT_ADAM; same convention):
//   u = scale*g;  m = beta1*m + (1-beta1)*u;  s = beta2*s + (1-beta2)*u*u
//   p += dt*((c1*m) / (c2*sqrt(s) + eps) - wd*p)
//   c1 = 1/(1-beta1^t), c2 = 1/sqrt(1-beta2^t), t the 1-based update count
// v (or m) and s are fp32 buckets in the flat layout of params; `vel` carries
// v under OPT_MOM and m under OPT_ADAM, `sq` carries s.  A conv-weight pad
// row has p = g = v = m = s = 0 and stays there under all three formulas
// (Adam: 0/(0 + eps) - wd*0).  OPT is a compile-time selector: the plain
// instantiations never see vel, sq or an argument struct, the momentum ones
// never see sq.
#ifndef PCNN_LAUNCH_H
#error "include pcnn_launch.h before sgd_update.h"
#endif

enum { OPT_PLAIN = 0, OPT_MOM = 1, OPT_ADAM = 2 };

struct MomArgs {
  float scale, dt, mu, wd;
  int nesterov;
};

// omb1, omb2: 1-beta1 and 1-beta2 as the host rounded them from double.
// 1.f - beta2 on the device would inherit the rounding of beta2 itself: at
// 0.999 that is 1.3e-5 relative on (1-beta2), which the first update turns
// into 6e-6 on the step.
struct AdamArgs {
  float scale, dt, beta1, beta2, eps, wd, c1, c2;
  float omb1, omb2;
};

// Kernel argument of the momentum kernels from the launcher's optimizer.
inline MomArgs mom_args(const pcnn_opt* opt) {
  return MomArgs{opt->scale, opt->dt, opt->mu, opt->wd, opt->nesterov};
}

// Kernel argument of the Adam kernels: mu carries beta1 (pcnn_launch.h).
inline AdamArgs adam_args(const pcnn_opt* opt) {
  return AdamArgs{opt->scale, opt->dt, opt->mu,   opt->beta2, opt->eps,
                  opt->wd,    opt->c1, opt->c2,   opt->omb1,  opt->omb2};
}

// Which kernels an optimizer selects (pcnn_launch.h): OPT_ADAM by kind,
// otherwise OPT_MOM by a velocity bucket, otherwise OPT_PLAIN.  -1: Adam
// without both of its state buckets.
inline int opt_select(const pcnn_opt* opt) {
  if (opt->kind == 1)
    return opt->vel != nullptr && opt->sq != nullptr ? OPT_ADAM : -1;
  return opt->vel != nullptr ? OPT_MOM : OPT_PLAIN;
}

// Loss scaling (DeepCNN only): the device-resident scaler state, eight
// 32-bit words behind pcnn_opt.ls_state.  scale, inv_scale, c1 and c2 are
// floats; found_inf, good_steps, skipped and t are int32 stored in place.
// t is the 1-based count of the update that c1, c2 belong to, the next one
// to be applied: t - 1 updates have been applied so far.
enum {
  LS_SCALE = 0,
  LS_INV_SCALE = 1,
  LS_FOUND_INF = 2,
  LS_GOOD_STEPS = 3,
  LS_SKIPPED = 4,
  LS_T = 5,
  LS_C1 = 6,
  LS_C2 = 7,
  LS_WORDS = 8
};

// LS is the fourth compile-time selector of an update site: false leaves
// the step and the argument struct as the launcher passed them.  true reads
// the state: the gradients in the bucket are scale x the true ones, so the
// plain step and the `scale` of the momentum and Adam forms are multiplied
// by inv_scale, and Adam takes c1, c2 from the state (its update count lives
// there, not on the host).  The update body itself is sgd_apply1/4 above all
// the same.
__device__ __forceinline__ bool ls_found_inf(const float* __restrict__ ls) {
  return reinterpret_cast<const int*>(ls)[LS_FOUND_INF] != 0;
}

__device__ __forceinline__ float ls_step(float step,
                                         const float* __restrict__ ls) {
  return step * ls[LS_INV_SCALE];
}

__device__ __forceinline__ MomArgs ls_args(MomArgs o,
                                           const float* __restrict__ ls) {
  o.scale *= ls[LS_INV_SCALE];
  return o;
}

__device__ __forceinline__ AdamArgs ls_args(AdamArgs o,
                                            const float* __restrict__ ls) {
  o.scale *= ls[LS_INV_SCALE];
  o.c1 = ls[LS_C1];
  o.c2 = ls[LS_C2];
  return o;
}

__device__ __forceinline__ float mom_apply(float p, float g, float& v,
                                           const MomArgs& o) {
  const float u = o.scale * g - o.wd * p;
  v = o.mu * v + u;
  return p + o.dt * (o.nesterov ? u + o.mu * v : v);
}

__device__ __forceinline__ void mom_apply4(float4& p, const float4& g,
                                           float4& v, const MomArgs& o) {
  p.x = mom_apply(p.x, g.x, v.x, o);
  p.y = mom_apply(p.y, g.y, v.y, o);
  p.z = mom_apply(p.z, g.z, v.z, o);
  p.w = mom_apply(p.w, g.w, v.w, o);
}

__device__ __forceinline__ float adam_apply(float p, float g, float& m,
                                            float& s, const AdamArgs& o) {
  const float u = o.scale * g;
  m = o.beta1 * m + o.omb1 * u;
  s = o.beta2 * s + o.omb2 * (u * u);
  return p + o.dt * ((o.c1 * m) / (o.c2 * sqrtf(s) + o.eps) - o.wd * p);
}

__device__ __forceinline__ void adam_apply4(float4& p, const float4& g,
                                            float4& m, float4& s,
                                            const AdamArgs& o) {
  p.x = adam_apply(p.x, g.x, m.x, s.x, o);
  p.y = adam_apply(p.y, g.y, m.y, s.y, o);
  p.z = adam_apply(p.z, g.z, m.z, s.z, o);
  p.w = adam_apply(p.w, g.w, m.w, s.w, o);
}

// Apply the update to parameter i and zero its gradient; returns the new
// parameter value.  Args is MomArgs (unused under OPT_PLAIN) or AdamArgs.
template <int OPT, typename idx_t, typename Args>
__device__ __forceinline__ float sgd_apply1(float* __restrict__ params,
                                            float* __restrict__ grads,
                                            float* __restrict__ vel,
                                            float* __restrict__ sq, idx_t i,
                                            float step, const Args& o) {
  float pnew;
  if constexpr (OPT == OPT_ADAM) {
    float m = vel[i], s = sq[i];
    pnew = adam_apply(params[i], grads[i], m, s, o);
    params[i] = pnew;
    vel[i] = m;
    sq[i] = s;
  } else if constexpr (OPT == OPT_MOM) {
    float v = vel[i];
    pnew = mom_apply(params[i], grads[i], v, o);
    params[i] = pnew;
    vel[i] = v;
  } else {
    params[i] += step * grads[i];
    pnew = params[i];
  }
  grads[i] = 0.f;
  return pnew;
}

// The same for the four parameters i .. i+3 (i a multiple of 4; the buckets
// are 16-byte aligned).
template <int OPT, typename Args>
__device__ __forceinline__ void sgd_apply4(float* __restrict__ params,
                                           float* __restrict__ grads,
                                           float* __restrict__ vel,
                                           float* __restrict__ sq, int i,
                                           float step, const Args& o) {
  float4 pv = *reinterpret_cast<float4*>(params + i);
  if constexpr (OPT == OPT_ADAM) {
    float4 mv = *reinterpret_cast<float4*>(vel + i);
    float4 sv = *reinterpret_cast<float4*>(sq + i);
    const float4 gv = *reinterpret_cast<float4*>(grads + i);
    adam_apply4(pv, gv, mv, sv, o);
    *reinterpret_cast<float4*>(params + i) = pv;
    *reinterpret_cast<float4*>(vel + i) = mv;
    *reinterpret_cast<float4*>(sq + i) = sv;
  } else if constexpr (OPT == OPT_MOM) {
    float4 vv = *reinterpret_cast<float4*>(vel + i);
    const float4 gv = *reinterpret_cast<float4*>(grads + i);
    mom_apply4(pv, gv, vv, o);
    *reinterpret_cast<float4*>(params + i) = pv;
    *reinterpret_cast<float4*>(vel + i) = vv;
  } else {
    const float4 gv = *reinterpret_cast<float4*>(grads + i);
    pv.x += step * gv.x;
    pv.y += step * gv.y;
    pv.z += step * gv.z;
    pv.w += step * gv.w;
    *reinterpret_cast<float4*>(params + i) = pv;
  }
  *reinterpret_cast<float4*>(grads + i) = make_float4(0.f, 0.f, 0.f, 0.f);
}

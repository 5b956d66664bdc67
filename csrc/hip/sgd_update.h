// The SGD update rule of every update kernel, device side.
//
// Included INSIDE the namespace of each .hip file (pcnn, pcnn_deep), after
// pcnn_launch.h: MomArgs is a kernel argument, so its namespace is part of
// the kernels' symbol names, which profiles and tools refer to.
//
// Plain (MOM = false):  p += step*g
// Momentum / Nesterov / weight decay (MOM = true; ascent convention, g as
// the plain form reads it):
//   u = scale*g - wd*p;  v = mu*v + u;  p += dt*v
//   nesterov:            p += dt*(u + mu*v)     (v the freshly updated one)
// v is the fp32 velocity bucket, same flat layout as params.  A conv-weight
// pad row has p = g = v = 0 and stays there under these formulas.  MOM is a
// compile-time flag: the plain instantiations never see vel or MomArgs.
#ifndef PCNN_LAUNCH_H
#error "include pcnn_launch.h before sgd_update.h"
#endif

struct MomArgs {
  float scale, dt, mu, wd;
  int nesterov;
};

// Kernel argument of the momentum kernels from the launcher's optimizer.
inline MomArgs mom_args(const pcnn_opt* opt) {
  return MomArgs{opt->scale, opt->dt, opt->mu, opt->wd, opt->nesterov};
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

// Apply the update to parameter i and zero its gradient; returns the new
// parameter value.
template <bool MOM, typename idx_t>
__device__ __forceinline__ float sgd_apply1(float* __restrict__ params,
                                            float* __restrict__ grads,
                                            float* __restrict__ vel, idx_t i,
                                            float step, const MomArgs& o) {
  float pnew;
  if constexpr (MOM) {
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
template <bool MOM>
__device__ __forceinline__ void sgd_apply4(float* __restrict__ params,
                                           float* __restrict__ grads,
                                           float* __restrict__ vel, int i,
                                           float step, const MomArgs& o) {
  float4 pv = *reinterpret_cast<float4*>(params + i);
  if constexpr (MOM) {
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

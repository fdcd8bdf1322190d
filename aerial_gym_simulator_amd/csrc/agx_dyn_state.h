#pragma once
// Env-step state access: the fdiv / fsqrt arithmetic switch, the per-env value structs (EnvState, Derived, Gains, Wrench), the SoA
// access layer (SoaRef, AGX_AT, AGX_QAT), the kernel-argument pinning (AGX_ARG_*, arg_pin) and load / store of state, derived and gains.
// Part of the one translation unit agx_dynamics.hip, which alone includes it (after the AGX_DYN_* switches).

namespace agx {
#if AGX_DYN_FAST_RCP
// one Newton step each: 1 ulp -> about 0.5 ulp (not correctly rounded, not meant to be), 3 / 4 instructions
AGX_DEV float srcp(float x) {
  float r = __builtin_amdgcn_rcpf(x);
  return fmaf(r, fmaf(-x, r, 1.0f), r);
}
AGX_DEV float fdiv(float a, float b) { return a * srcp(b); }
AGX_DEV float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
#else
AGX_DEV float fdiv(float a, float b) { return a / b; }
AGX_DEV float fsqrt(float x) { return sqrtf(x); }
#endif
// v / |v| the way torch evaluates it: the norm first, then one division per component
AGX_DEV V3 normalized(V3 v) {
  float nv = norm(v);
  return V3{fdiv(v.x, nv), fdiv(v.y, nv), fdiv(v.z, nv)};
}
}  // namespace agx

namespace agx {
struct EnvState {
  V3 p;
  Q4 q;
  V3 v, w;
};
struct Derived {
  V3 euler;
  Q4 qveh;
  V3 vveh, vbody, wbody;
};
struct Gains {
  V3 kp, kv, kr, kw;
};
struct Wrench {
  V3 f, t;
};


// SoA element (component c of env i): uniform column base (scalar unit) + one 32-bit byte offset per lane,
// i.e. the `global_load v, v_off, s[base]` addressing form instead of a 64-bit VGPR address per access.
// Round 4: as a BUFFER access -- `buffer_load_dword v, v_off, s[descriptor], s_column offen`: the array's base in a 128-bit
// descriptor (scalar registers, rebuilt where it is used: four scalar instructions), the column offset c n sizeof(T) in a scalar
// register, the lane's part i sizeof(T) in ONE vector register shared by every access of the kernel.  The pointer form above
// compiles to that `global_load v, v_off, s[base]` only when the instruction selector finds the offset's 32 -> 64-bit extension
// in the access's own basic block; behind any run-time condition it does not, and each access cost a 64-bit vector add and a
// register pair: 288 of the ~2500 vector instructions of k_env_step<4, position, single> and its largest block of live registers
// (profiles/r04_at_scale_experiments.txt).  n x 16 columns x 4 bytes < 2^32.
template <class T>
struct SoaRef {
  static_assert(sizeof(T) == 4, "32-bit elements");
  T *base;
  unsigned col_bytes, lane_bytes;
  AGX_DEV __amdgpu_buffer_rsrc_t rsrc() const {
    // raw buffer (stride 0), every offset in range, gfx9 data format word (composable_kernel: CK_BUFFER_RESOURCE_3RD_DWORD)
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<typename std::remove_const<T>::type *>(base), 0, -1, 0x00020000);
  }
  AGX_DEV operator typename std::remove_const<T>::type() const {
    return __builtin_bit_cast(typename std::remove_const<T>::type,
                              __builtin_amdgcn_raw_buffer_load_b32(rsrc(), (int)lane_bytes, (int)col_bytes, 0));
  }
  AGX_DEV void operator=(typename std::remove_const<T>::type v) const {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), rsrc(), (int)lane_bytes, (int)col_bytes, 0);
  }
};
template <class T>
AGX_DEV SoaRef<T> soa_at(T *base, int c, int n, int i) {
  return SoaRef<T>{base, (unsigned)c * (unsigned)n * (unsigned)sizeof(T), (unsigned)i * (unsigned)sizeof(T)};
}
#define AGX_AT(p, c) agx::soa_at((p), (c), n, i)
// The lane-quad kernels index a column by the lane's component (c0 + l): the per-lane part of the address, (l n + i) sizeof(T),
// is computed ONCE as a 32-bit byte offset (n <= 65536 there) and every access is scalar column base + that offset -- instead of
// a 64-bit multiply-add and two 64-bit adds on the vector unit per access, in front of the kernel's first load.
template <class T>
AGX_DEV T &soa_at_off(T *base, int c, int n, unsigned off_bytes) {
  T *col = base + (ptrdiff_t)c * (ptrdiff_t)n;
  return *reinterpret_cast<T *>(reinterpret_cast<char *>(const_cast<typename std::remove_const<T>::type *>(col)) + (size_t)off_bytes);
}
// (Stays the pointer form: as buffer accesses the 8192-env step was 3 % SLOWER -- 12.8 vs 12.4 us, measured -- these kernels run
//  one wave per SIMD and are bound by that wave's own instruction chain, to which the descriptor set-up and the extra branches of
//  the `pointer ? load : uniform` arms add; the one-lane kernels are bound by throughput and registers, where they pay.)
#define AGX_QAT(p, c, off) agx::soa_at_off((p), (c), n, (off))

// Kernel arguments of the position-step kernels, fetched as ONE batch per wave.  A kernel-argument field is a load from constant
// memory that the compiler emits where the field is used: in a kernel of many basic blocks that is one s_load and one
// `s_waitcnt lgkmcnt(0)` -- a full scalar-memory round trip that a lone wave per SIMD sits out -- in nearly every block, one in
// front of nearly every group of stores.  arg_pin() reads the field HERE and passes it through an empty volatile asm that takes
// and returns it in scalar registers: the compiler cannot re-load it later (it no longer knows where the value came from) and
// cannot sink the asm, so the fields pinned back to back at the top of a wave are fetched by a few wide s_loads under one wait
// and live in SGPRs from there.  A pointer is pinned as a GLOBAL-address-space pointer: what the compiler knows about a pointer
// kernel argument and would not know about an opaque 64-bit value (a generic pointer: flat_load / flat_store).
// The fetch is written in two passes over one list of fields -- every field read into a local, then every local pinned -- because
// the pins keep their order and a read placed between two pins is issued behind the wait of the first: a second round trip.
// 
#define AGX_ARG_READ(S, f) auto S##_##f = S##0 .f;
#define AGX_ARG_READ_N(S, f, N) \
  float S##_##f[N];             \
  _Pragma("unroll") for (int k_ = 0; k_ < N; ++k_) S##_##f[k_] = S##0 .f[k_];
#define AGX_ARG_PIN(S, f) \
  arg_pin(S##_##f);       \
  S.f = S##_##f;
#define AGX_ARG_PIN_N(S, f, N) \
  _Pragma("unroll") for (int k_ = 0; k_ < N; ++k_) { arg_pin(S##_##f[k_]); S.f[k_] = S##_##f[k_]; }
template <class T>
AGX_DEV void arg_pin(T &x) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two scalar registers");
  asm volatile("" : "+s"(x));
}
template <class T>
AGX_DEV void arg_pin(T *&p) {
  typedef T __attribute__((address_space(1))) *global_ptr;
  global_ptr g = (global_ptr)p;
  asm volatile("" : "+s"(g));
  p = (T *)g;
}
// a relaxed atomic load of the narrowest scope: an ordinary global_load that stays one (never merged with another load)
AGX_DEV float gain_load(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
template <class T, int N>
AGX_DEV void arg_pin(T (&a)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) arg_pin(a[k]);
}

AGX_DEV EnvState load_state(const float *__restrict__ s, int n, int i) {
  EnvState e;
  e.p = V3{AGX_AT(s, 0), AGX_AT(s, 1), AGX_AT(s, 2)};
  e.q = Q4{AGX_AT(s, 3), AGX_AT(s, 4), AGX_AT(s, 5), AGX_AT(s, 6)};
  e.v = V3{AGX_AT(s, 7), AGX_AT(s, 8), AGX_AT(s, 9)};
  e.w = V3{AGX_AT(s, 10), AGX_AT(s, 11), AGX_AT(s, 12)};
  return e;
}
AGX_DEV void store_state(float *__restrict__ s, int n, int i, const EnvState &e) {
  AGX_AT(s, 0) = e.p.x; AGX_AT(s, 1) = e.p.y; AGX_AT(s, 2) = e.p.z;
  AGX_AT(s, 3) = e.q.x; AGX_AT(s, 4) = e.q.y; AGX_AT(s, 5) = e.q.z; AGX_AT(s, 6) = e.q.w;
  AGX_AT(s, 7) = e.v.x; AGX_AT(s, 8) = e.v.y; AGX_AT(s, 9) = e.v.z;
  AGX_AT(s, 10) = e.w.x; AGX_AT(s, 11) = e.w.y; AGX_AT(s, 12) = e.w.z;
}
AGX_DEV void store_derived(float *__restrict__ d, int n, int i, const Derived &x) {
  AGX_AT(d, 0) = x.euler.x; AGX_AT(d, 1) = x.euler.y; AGX_AT(d, 2) = x.euler.z;
  AGX_AT(d, 3) = x.qveh.x; AGX_AT(d, 4) = x.qveh.y; AGX_AT(d, 5) = x.qveh.z; AGX_AT(d, 6) = x.qveh.w;
  AGX_AT(d, 7) = x.vveh.x; AGX_AT(d, 8) = x.vveh.y; AGX_AT(d, 9) = x.vveh.z;
  AGX_AT(d, 10) = x.vbody.x; AGX_AT(d, 11) = x.vbody.y; AGX_AT(d, 12) = x.vbody.z;
  AGX_AT(d, 13) = x.wbody.x; AGX_AT(d, 14) = x.wbody.y; AGX_AT(d, 15) = x.wbody.z;
}
AGX_DEV void store_body_velocities(float *__restrict__ d, int n, int i, const Derived &x) {
  AGX_AT(d, 10) = x.vbody.x; AGX_AT(d, 11) = x.vbody.y; AGX_AT(d, 12) = x.vbody.z;
  AGX_AT(d, 13) = x.wbody.x; AGX_AT(d, 14) = x.wbody.y; AGX_AT(d, 15) = x.wbody.z;
}
AGX_DEV Derived load_derived(const float *__restrict__ d, int n, int i) {
  Derived x;
  x.euler = V3{AGX_AT(d, 0), AGX_AT(d, 1), AGX_AT(d, 2)};
  x.qveh = Q4{AGX_AT(d, 3), AGX_AT(d, 4), AGX_AT(d, 5), AGX_AT(d, 6)};
  x.vveh = V3{AGX_AT(d, 7), AGX_AT(d, 8), AGX_AT(d, 9)};
  x.vbody = V3{AGX_AT(d, 10), AGX_AT(d, 11), AGX_AT(d, 12)};
  x.wbody = V3{AGX_AT(d, 13), AGX_AT(d, 14), AGX_AT(d, 15)};
  return x;
}
AGX_DEV Gains uniform_gains(const AgxRobotParams &P) {
  Gains k;
  k.kp = V3{P.gains_uniform[0], P.gains_uniform[1], P.gains_uniform[2]};
  k.kv = V3{P.gains_uniform[3], P.gains_uniform[4], P.gains_uniform[5]};
  k.kr = V3{P.gains_uniform[6], P.gains_uniform[7], P.gains_uniform[8]};
  k.kw = V3{P.gains_uniform[9], P.gains_uniform[10], P.gains_uniform[11]};
  return k;
}
AGX_DEV Gains load_gains(const float *__restrict__ g, int n, int i) {
  Gains k;
  k.kp = V3{AGX_AT(g, 0), AGX_AT(g, 1), AGX_AT(g, 2)};
  k.kv = V3{AGX_AT(g, 3), AGX_AT(g, 4), AGX_AT(g, 5)};
  k.kr = V3{AGX_AT(g, 6), AGX_AT(g, 7), AGX_AT(g, 8)};
  k.kw = V3{AGX_AT(g, 9), AGX_AT(g, 10), AGX_AT(g, 11)};
  return k;
}
}  // namespace agx

// region/wave.h -- wave-level primitives: ballot64, L2 (agent-scope) loads / stores and fences, uni / uglobal (wave-uniform values onto the scalar unit), mbcnt, min8 / sum8 (DPP over
// 8-lane groups), rl / rlf (lane broadcast), pack_xy, lget / lset (the region list: LDS ring G_LST, older entries in RCtx::spill), angle_diff (myLSD.cpp:540-542 / :1009-1011).
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// a load that does not stop at the CU's vector cache: for words other wavefronts change with ATOMICS (performed in L2, they leave a
// stale line in the L1 behind; plain stores of the same CU do not)
__device__ __forceinline__ uint32_t ld_l2(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void wg_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }
// words shared with OTHER workgroups (the help protocol of the seed loop): written and read in L2, ordered by agent-scope fences
__device__ __forceinline__ void st_l2(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void agent_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); }
__device__ __forceinline__ void agent_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }

// Function arguments arrive in vector registers even when they are the same in every lane; the inner loop wants them on
// the scalar unit (scalar compares and branches, SGPR-base addressing of global memory with 32-bit lane offsets).
#define AS1 __attribute__((address_space(1)))
typedef float nf4 __attribute__((ext_vector_type(4)));       // (HIP's float4 class cannot be reached through an address-space pointer)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
template <class T>
__device__ __forceinline__ AS1 T* uglobal(T* p) {
    const unsigned long long v = (unsigned long long)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (AS1 T*)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int mbcnt(unsigned long long m) {   // number of set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// minimum over the 8 lanes of a group (lane >> 3), every lane gets it: three DPP steps, no LDS traffic
__device__ __forceinline__ float min8(float v) {
    int t = __float_as_int(v);
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(t, t, 0xB1, 0xf, 0xf, false)));   // quad_perm [1,0,3,2]
    t = __float_as_int(v);
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(t, t, 0x4E, 0xf, 0xf, false)));   // quad_perm [2,3,0,1]
    t = __float_as_int(v);
    v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(t, t, 0x141, 0xf, 0xf, false)));  // row_half_mirror
    return v;
}

// sum over the 8 lanes of a group, every lane gets it (used where at most one lane holds a non-zero value: the sum is that value)
__device__ __forceinline__ float sum8(float v) {
    int t = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(t, t, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    t = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(t, t, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    t = __float_as_int(v);
    v += __int_as_float(__builtin_amdgcn_update_dpp(t, t, 0x141, 0xf, 0xf, false));  // row_half_mirror
    return v;
}

__device__ __forceinline__ double rl(double v, int l) {  // broadcast lane l (l wave-uniform)
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, l);
    hi = __builtin_amdgcn_readlane(hi, l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float rlf(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ uint32_t pack_xy(int x, int y) { return ((uint32_t)y << 16) | (uint32_t)x; }
__device__ __forceinline__ uint32_t lget(const RCtx& c, int i) { return i >= c.llo ? G_LST(c.wave)[i & LMASK] : c.spill[i]; }
__device__ __forceinline__ void lset(const RCtx& c, int i, uint32_t v) {           // (after the grow: every entry has one home)
    if (i >= c.llo) G_LST(c.wave)[i & LMASK] = v; else c.spill[i] = v;
}
__device__ __forceinline__ double angle_diff(double a, double b) {  // myLSD.cpp:540-542 / :1009-1011
    double d = fabs(a - b);
    if (d > kPi * 3 / 2.0) d = fabs(d - 2.0 * kPi);
    return d;
}

// The arguments of one evaluation, and the ONE parameter list of every kernel that takes them (included by defect_dims.h).
//
// Host code fills an EvalArgs.  A kernel does not take that struct: its parameter list is ASSET_EVAL_PARAMS -- the fields a wave needs
// before it can address its first load as leading scalar parameters, in order of need, then the rest by value as one EvalCold -- and its
// first statement, ASSET_EVAL_REBUILD, forms a local `const EvalArgs a` from them again.  gfx950 delivers the leading parameters in user
// SGPRs when the wave is launched (kernel-argument preload, build.py: KERNARG_PRELOAD); everything behind them is read from the
// kernel-argument segment by scalar loads, which miss every cache at the start of a dispatch.  The hot list ends where the user SGPRs do:
// 16 of them, two taken by the segment's address, so 14 dwords -- ten parameters.  Compiled without the option the same list is loaded
// from the segment like any other: only the signature is ABI.
//
// eval_args_pack() is the only writer of a launch's argument values and eval_args_rebuild() their only reader; EvalKernArgs has the layout of
// the kernel-argument segment (natural alignment, parameters in order), which tests/test_kernarg_layout_cpu.py holds against the metadata of
// every compiled kernel.  Plain C++: no HIP header, so that host programs without a device compiler can include it.
#pragma once
#include <cstddef>

#if defined(__HIP__) || defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define ASSET_HOST_DEVICE __host__ __device__
#else
#define ASSET_HOST_DEVICE
#endif

namespace asset_hip {

struct EvalArgs {
  int nseg;
  const double* X;     // NLP primal vector (device)
  const double* L;     // equality multipliers (device); unused for value-only
  const int* vindex;   // [IR x nseg] column-major (device)
  const int* cindex;   // [OR x nseg] column-major (device)
  double* FX;          // [nseg x OR] blocks or null
  double* AGX;         // [nseg x IR] blocks or null
  double* KKT;         // [nseg x KSTRIDE] blocks (layout: Dims::KL below) or null
  double* work;        // [grid][G][SLOT] per-workgroup ODE result slots (L2-resident scratch in HBM)
  // On-device assembly (dense stage, ASM kernels): KKT entries go into the solver's value array instead of being
  // stored as blocks (DenseFunctionBase.h:1413-1523 KKTFillAll / KKTFillJac; locations NonLinearProgram.cpp:316-330;
  // the reference serialises clashing columns with mutexes, KKTClashes / KKTLocks).  kmap holds, per segment and in
  // accumulator-fragment order, one entry per lane and accumulator entry:  m >= 0 -- value location used by this slot
  // alone: the entry is STORED (the caller hands over zeros there, as the reference zeroes the KKT values before every
  // evaluation, PSIOPT.cpp:107);  m <= -2 -- location -(m+2) is shared with other slots of this constraint (boundary
  // nodes of adjacent segments, phase parameters): no-return f64 atomic add;  -1 -- no KKT slot.  In accumulate mode
  // every slot is encoded as shared, which makes the evaluation a true += at about 1.4e11 atomics/s.
  const int* kmap = nullptr;
  double* values = nullptr;
  // Locations that three or more slots share (entries between phase parameters: one contribution per segment) are not
  // added to atomically -- the order of the additions, hence the last bits of the sum, would change from run to run --
  // but STAGED: the map names such a location as nvalues + k, slot k of `stage`, every staged slot owns one cell, and
  // asm_reduce_kernel sums the cells of each location in slot order afterwards (capi.hip).  Locations with exactly two
  // contributors (boundary nodes of adjacent segments) keep the atomic: a + b = b + a, bit for bit.
  double* stage = nullptr;
  int nvalues = 0;
  // per-lane constants of the dense stage, computed once per handle (defect_kernels.h: LaneConsts, lane_setup_kernel)
  const void* lane_consts = nullptr;
  const void* lane_consts_res = nullptr;   // the record of the resident kernel (defect_resident.h: ResLane)
  // Index tables whose rows are runs -- vindex[s][k] = aff_v0 + s aff_vs + k, cindex[s][k] = aff_c0 + s aff_cs + k, what a
  // phase without BlockConstant controls and ODE parameters produces (PhaseIndexer.cpp:361-372, 179-189) -- are recognised
  // when the handle is created: the resident kernel then forms the addresses of z and lam itself instead of loading them
  // (one dependent memory round trip less at the start of every wave).
  int affine = 0, aff_v0 = 0, aff_vs = 0, aff_c0 = 0, aff_cs = 0;
  // plain functions (func_kernels.h): constants of every application, [nseg][F::NACONST] (vf.ApplConst) or null
  const double* appl_consts = nullptr;
  // bit 0 (ASSET_HIP_KEEP_HESSIAN_SLOTS, Jacobian kinds): the Hessian slots of the KKT blocks are not written at all
  // instead of being written as zeros -- KKTFillJac (DenseFunctionBase.h:1468-1523) never reads them
  int flags = 0;
  // Heavy right-hand sides: segments per group of the unit kernels that wrote the workspace slots (0: unknown).  The dense
  // part behind them then takes every group's segments on the XCD whose L2 holds them (defect_resident.h, GIVEN).
  int units_gp = 0;
  // Workgroups (grid x) of the launch that carries these arguments: the launcher's value (eval_args_pack), never the caller's.  The
  // resident kernel splits the mesh by it -- gridDim.x would be a load from the hidden arguments at the head of every wave.
  int nwg = 0;
};

// What a kernel reads only after its first loads are under way: one by-value struct behind the hot parameters.
struct EvalCold {
  const int* vindex;
  const int* cindex;
  double* AGX;
  double* work;
  const int* kmap;
  double* values;
  double* stage;
  const void* lane_consts;
  const void* lane_consts_res;
  const double* appl_consts;
  int nvalues, flags, units_gp;
};

// The hot parameters in order of need, none straddling an 8-byte boundary: X, L, nseg, the workgroups of the launch with `affine` as
// its sign bit, the four run constants, then the output pointers as far as the user SGPRs reach.
#define ASSET_EVAL_HOT_PARAMS 10      // parameters ...
#define ASSET_EVAL_HOT_DWORDS 14      // ... and dwords of the hot list
// The preload is a compiler option (build.py: KERNARG_PRELOAD), so the sources cannot turn it off; the switch says which build this
// is -- tools/build_one.py drops the option when it sees -DASSET_KERNARG_PRELOAD=0 -- and with it what a kernel descriptor must say.
#ifndef ASSET_KERNARG_PRELOAD
#define ASSET_KERNARG_PRELOAD 1
#endif
#define ASSET_EVAL_PRELOAD_DWORDS (ASSET_KERNARG_PRELOAD ? ASSET_EVAL_HOT_DWORDS : 0)   // .amdhsa_user_sgpr_kernarg_preload_length
#define ASSET_EVAL_PARAMS                                                                                                         \
  const double* ka_X, const double* ka_L, int ka_nseg, int ka_nwg_affine, int ka_aff_v0, int ka_aff_vs, int ka_aff_c0,             \
      int ka_aff_cs, double* ka_KKT, double* ka_FX, ::asset_hip::EvalCold ka_cold
#define ASSET_EVAL_REBUILD                                                                                                        \
  const ::asset_hip::EvalArgs a = ::asset_hip::eval_args_rebuild(ka_X, ka_L, ka_nseg, ka_nwg_affine, ka_aff_v0, ka_aff_vs,        \
                                                                 ka_aff_c0, ka_aff_cs, ka_KKT, ka_FX, ka_cold);

// The kernel-argument segment of ASSET_EVAL_PARAMS, member for parameter.
struct EvalKernArgs {
  const double* X;
  const double* L;
  int nseg, nwg_affine, aff_v0, aff_vs, aff_c0, aff_cs;
  double* KKT;
  double* FX;
  EvalCold cold;
};
constexpr int kEvalParams = ASSET_EVAL_HOT_PARAMS + 1;     // entries of a launch's argument-pointer array that eval_args_pack fills
static_assert(offsetof(EvalKernArgs, KKT) == 40 && offsetof(EvalKernArgs, cold) == 4 * ASSET_EVAL_HOT_DWORDS,
              "the hot list: ASSET_EVAL_HOT_DWORDS dwords without padding");

// a -> the argument values of a launch of `nwg` workgroups, and the pointer to each in parameter order (hipLaunchKernel /
// hipModuleLaunchKernel take such an array; a kernel's own trailing parameters follow at ptrs[kEvalParams])
inline void eval_args_pack(const EvalArgs& a, unsigned nwg, EvalKernArgs& k, void** ptrs) {
  k.X = a.X, k.L = a.L, k.nseg = a.nseg;
  k.nwg_affine = int((nwg & 0x7fffffffu) | (a.affine ? 0x80000000u : 0u));
  k.aff_v0 = a.aff_v0, k.aff_vs = a.aff_vs, k.aff_c0 = a.aff_c0, k.aff_cs = a.aff_cs;
  k.KKT = a.KKT, k.FX = a.FX;
  k.cold = EvalCold{a.vindex, a.cindex, a.AGX, a.work, a.kmap, a.values, a.stage, a.lane_consts, a.lane_consts_res, a.appl_consts,
                    a.nvalues, a.flags, a.units_gp};
  void* const p[kEvalParams] = {&k.X, &k.L, &k.nseg, &k.nwg_affine, &k.aff_v0, &k.aff_vs, &k.aff_c0, &k.aff_cs, &k.KKT, &k.FX, &k.cold};
  for (int i = 0; i < kEvalParams; i++) ptrs[i] = p[i];
}

ASSET_HOST_DEVICE inline EvalArgs eval_args_rebuild(const double* X, const double* L, int nseg, int nwg_affine, int aff_v0, int aff_vs,
                                                    int aff_c0, int aff_cs, double* KKT, double* FX, const EvalCold& c) {
  EvalArgs a;
  a.nseg = nseg, a.X = X, a.L = L, a.vindex = c.vindex, a.cindex = c.cindex, a.FX = FX, a.AGX = c.AGX, a.KKT = KKT, a.work = c.work;
  a.kmap = c.kmap, a.values = c.values, a.stage = c.stage, a.nvalues = c.nvalues;
  a.lane_consts = c.lane_consts, a.lane_consts_res = c.lane_consts_res;
  a.affine = nwg_affine < 0 ? 1 : 0, a.aff_v0 = aff_v0, a.aff_vs = aff_vs, a.aff_c0 = aff_c0, a.aff_cs = aff_cs;
  a.appl_consts = c.appl_consts, a.flags = c.flags, a.units_gp = c.units_gp;
  a.nwg = nwg_affine & 0x7fffffff;
  return a;
}

}  // namespace asset_hip

// Kernel registry: every (ODE functor, transcription mode, blocked) instantiation compiled into libasset_hip.so registers
// one entry; so does every module compiled at run time (capi.hip: asset_hip_jit_plugin).  The C ABI (capi.hip) looks
// entries up by name at create time.  An entry is data -- the integers of kernel_meta.h and one reference per kernel
// variant -- and ONE planner and launcher (plan_lgl, launch_plan below) serve the kernels linked into the library (host stubs) and the
// kernels of a run-time module (hipFunction_t) alike.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "kernel_meta.h"
#include "integ_kernels.h"
#include "interp_kernels.h"
#include "mesh_kernels.h"
#include "propagate_kernels.h"

namespace asset_hip {

// ---- kernel references ---------------------------------------------------------------------------------------------
// A module compiled at run time: the code object and the lowered kernel names stay with it, and it is loaded on every
// device it is used on -- a hipModule_t (and its hipFunction_t handles) belongs to the device that was current when it
// was loaded, while a handle of the C ABI may live on any device (asset_hip_defect_desc::device).  Loading is lazy: the
// first launch on a device loads the code object there.
struct RtcModule {
  std::vector<char> code;
  std::vector<std::pair<int, std::string>> names;   // (kernel slot, lowered name)
  struct PerDevice {
    hipModule_t mod = nullptr;
    std::vector<hipFunction_t> fn;                  // by kernel slot
  };
  std::mutex m;
  std::vector<PerDevice> dev;                       // by device ordinal; sized ONCE (hipGetDeviceCount) and never resized
  ~RtcModule() {
    for (auto& pd : dev)
      if (pd.mod) (void)hipModuleUnload(pd.mod);
  }
  // kernel `slot` on the CURRENT device (loads the module there at first use).  The function handle is copied out under the
  // lock: no pointer into `dev` outlives it.
  hipError_t on_current_device(int slot, hipFunction_t* out) {
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(m);
    if (dev.empty()) {
      int nd = 0;
      if ((e = hipGetDeviceCount(&nd)) != hipSuccess) return e;
      dev.resize(nd > d + 1 ? nd : d + 1);
    }
    if (d >= int(dev.size())) return hipErrorInvalidDevice;
    PerDevice& pd = dev[d];
    if (!pd.mod) {
      hipModule_t mod = nullptr;
      if ((e = hipModuleLoadData(&mod, code.data())) != hipSuccess) return e;
      int nslot = 0;
      for (auto& n : names) nslot = n.first + 1 > nslot ? n.first + 1 : nslot;
      std::vector<hipFunction_t> fn(nslot, nullptr);
      for (auto& n : names)
        if ((e = hipModuleGetFunction(&fn[n.first], mod, n.second.c_str())) != hipSuccess) {
          hipModuleUnload(mod);
          return e;
        }
      pd.fn.swap(fn);
      pd.mod = mod;
    }
    if (slot < 0 || slot >= int(pd.fn.size()) || !pd.fn[slot]) return hipErrorInvalidDeviceFunction;
    *out = pd.fn[slot];
    return hipSuccess;
  }
  // the module handle of the current device (loaded if need be): for reading the module's constants
  hipError_t module_on_current_device(hipModule_t* out) {
    int first = -1;
    for (auto& n : names) { first = n.first; break; }
    hipFunction_t f = nullptr;
    if (first >= 0) {
      hipError_t e = on_current_device(first, &f);
      if (e != hipSuccess) return e;
    }
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(m);
    if (d >= int(dev.size()) || !dev[d].mod) return hipErrorInvalidValue;
    *out = dev[d].mod;
    return hipSuccess;
  }
};

struct KRef {
  const void* host = nullptr;   // host stub of a kernel linked into this process (hipLaunchKernel)
  RtcModule* rtc = nullptr;     // kernel `slot` of a run-time module (hipModuleLaunchKernel on the current device)
  int slot = -1;
  explicit operator bool() const { return host || rtc; }
};
inline hipError_t klaunch(const KRef& k, dim3 grid, dim3 block, size_t shmem, hipStream_t st, void** args) {
  if (k.rtc) {
    hipFunction_t fn = nullptr;
    hipError_t e = k.rtc->on_current_device(k.slot, &fn);
    if (e != hipSuccess) return e;
    return hipModuleLaunchKernel(fn, grid.x, grid.y, grid.z, block.x, block.y, block.z, unsigned(shmem), st, args, nullptr);
  }
  if (!k.host) return hipErrorInvalidDeviceFunction;
  if (shmem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(k.host, hipFuncAttributeMaxDynamicSharedMemorySize, int(shmem));
    if (e != hipSuccess) return e;
  }
  return hipLaunchKernel(k.host, grid, block, args, shmem, st);
}

// ---- the kernels of a table: ONE list --------------------------------------------------------------------------------------
// X(slot, family, condition, kernel template, trailing template arguments...).  The family says what precedes the trailing
// arguments -- LGLG: <Ode, SCH, BLOCKED, G, ...>, LGL: <Ode, SCH, BLOCKED, ...>, NONE: <...> (all three: transcriptions of an ODE),
// ODE: <Ode, ...> (kernels of the ODE alone, whatever the transcription: they live in ONE entry per ODE, prop_home below),
// FUNC: <F, ...> (plain functions), BUNDLE: <..., Fs...> (bundles, run-time modules only), ODEEV: <Ode, Ev, ...> (an ODE with an event
// functor, run-time modules only: rtc_device.h, ASSET_RTC_PROP_EVENTS), ODECTL: <Ode, Ctl, ...> (an ODE with its control law, run-time
// modules only: ASSET_RTC_PROP_CTRL), ODEEVS: <Ode, Ev, ...> (an ODE with an event functor, propagated with its STM, run-time modules
// only: ASSET_RTC_PROP_EVENTS_STM) -- and the condition is the compile-time
// one (D = Dims<Ode, SCH, BLOCKED>) under which a shape linked into the library has the kernel.  The slot enum, the static tables
// (lgl_static_table, func_static_table) and the name expressions of a run-time module (rtc_kernel_expr, which names every slot of
// its kind: rtc_device.h compiles the variants a shape lacks to empty kernels) are all generated from this list.
// The propagation kernels depend on the ODE only.  They are compiled into, and looked up through, exactly one entry per ODE: its
// LGL3 transcription (id 2) with controls that are not BlockConstant -- every ODE that has any entry can have that one (the smallest
// scheme; an ODE without controls has no BlockConstant entries at all).  The rule is written here and nowhere else: the static
// tables, the name expressions of a run-time module and the C ABI's look-up (capi.hip: prop_entry) all call it.
constexpr int PROP_HOME_MODE = 2;
constexpr bool prop_home(int sch, bool blocked) { return sch == PROP_HOME_MODE && !blocked; }

#define ASSET_KERNELS(X)                                                                                                        \
  /* defect_kernels.h: ODE stage (S1), dense stage (S2), both in one launch (S3), ... as two-wave workgroups (S4) */            \
  X(K_LGL1_S1, LGLG, true, lgl_defect_kernel, 1, 1, false)                                                                      \
  X(K_LGL2_S1, LGLG, true, lgl_defect_kernel, 2, 1, false)                                                                      \
  X(K_LGL1_S2, LGLG, !D::WIDE, lgl_defect_kernel, 1, 2, false)                                                                  \
  X(K_LGL1_S2_ASM, LGLG, !D::WIDE, lgl_defect_kernel, 1, 2, true)                                                               \
  X(K_LGL2_S2, LGLG, !D::WIDE, lgl_defect_kernel, 2, 2, false)                                                                  \
  X(K_LGL2_S2_ASM, LGLG, !D::WIDE, lgl_defect_kernel, 2, 2, true)                                                               \
  X(K_LGL1_S3, LGLG, !D::WIDE && D::FUSED, lgl_defect_kernel, 1, 3, false)                                                      \
  X(K_LGL1_S3_ASM, LGLG, !D::WIDE && D::FUSED, lgl_defect_kernel, 1, 3, true)                                                   \
  X(K_LGL2_S3, LGLG, !D::WIDE && D::FUSED, lgl_defect_kernel, 2, 3, false)                                                      \
  X(K_LGL2_S3_ASM, LGLG, !D::WIDE && D::FUSED, lgl_defect_kernel, 2, 3, true)                                                   \
  X(K_LGL2_S4, LGLG, !D::WIDE && D::FUSED2, lgl_defect_kernel, 2, 4, false)                                                     \
  X(K_LANE_SETUP1, LGL, !D::WIDE, lane_setup_kernel, 1)                                                                         \
  X(K_LANE_SETUP2, LGL, !D::WIDE, lane_setup_kernel, 2)                                                                         \
  /* wide shapes: dense stage of four-wave workgroups (defect_wide.h); by output rows, no matrix instructions (defect_rows.h) */ \
  X(K_WIDE1, LGL, D::WIDE, lgl_wide_dense_kernel, 1, false)                                                                     \
  X(K_WIDE1_ASM, LGL, D::WIDE, lgl_wide_dense_kernel, 1, true)                                                                  \
  X(K_WIDE2, LGL, D::WIDE, lgl_wide_dense_kernel, 2, false)                                                                     \
  X(K_WIDE2_ASM, LGL, D::WIDE, lgl_wide_dense_kernel, 2, true)                                                                  \
  X(K_WIDE_SETUP, LGL, D::WIDE, wide_setup_kernel)                                                                              \
  X(K_ROWS1, LGL, D::WIDE && RowsDims<D>::OK, lgl_rows_kernel, 1)                                                               \
  X(K_ROWS2, LGL, D::WIDE && RowsDims<D>::OK, lgl_rows_kernel, 2)                                                               \
  /* value + adjoint gradient without a Jacobian; value only: the same kernel without its gradient parts (defect_adjgrad.h) */  \
  X(K_ADJGRAD, LGL, true, lgl_adjgrad_kernel, true)                                                                             \
  X(K_VALUE, LGL, true, lgl_adjgrad_kernel, false)                                                                              \
  /* resident single launch (defect_resident.h): one group per wave (RES), looped over groups (RESL), looped level-2 blocks as  \
     two-wave workgroups with the row-wise dense part (RESLP: defect_rowdpp.h), one group with the row-wise dense part of a     \
     shape that defaults to tiles (RES_ALT), the dense part alone over the slots the unit kernels wrote (RESD) */               \
  X(K_RES1, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 1, false)                                                     \
  X(K_RES1_ASM, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 1, true)                                                  \
  X(K_RES2, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 2, false)                                                     \
  X(K_RES2_ASM, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 2, true)                                                  \
  X(K_RESL1, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 1, false, true)                                              \
  X(K_RESL1_ASM, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 1, true, true)                                           \
  X(K_RESL2, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 2, false, true)                                              \
  X(K_RESL2_ASM, LGL, !D::WIDE && ResDims<D>::OK, lgl_resident_kernel, 2, true, true)                                           \
  X(K_RESLP, LGL, !D::WIDE && ResDims<D>::OK && ResDims<D>::LOOP_PAIR, lgl_resident_kernel, 2, false, true, false, true)        \
  X(K_RES_ALT, LGL, !D::WIDE && ResDims<D>::OK && ResDims<D>::RD_ALT, lgl_resident_kernel, 2, false, false, false, false, 1)    \
  X(K_RESD, LGL, !D::WIDE && ResDims<D>::GIVEN_OK, lgl_resident_kernel, 2, false, true, true)                                   \
  X(K_RESD_ASM, LGL, !D::WIDE && ResDims<D>::GIVEN_OK, lgl_resident_kernel, 2, true, true, true)                                \
  X(K_RES_SETUP, LGL, !D::WIDE && (ResDims<D>::OK || ResDims<D>::GIVEN_OK), res_lane_setup_kernel)                              \
  /* heavy right-hand sides, one wave per output unit (defect_units.h): interior units, cardinal units, the ODE stage of the    \
     Jacobian kinds (PHASE 3), interior and cardinal units in one launch (PHASE 4) */                                           \
  X(K_UNITS0, LGL, (Ode::NUNITS > 1), lgl_ode_units_kernel, 0)                                                                  \
  X(K_UNITS1, LGL, (Ode::NUNITS > 1), lgl_ode_units_kernel, 1)                                                                  \
  X(K_UNITSJ, LGL, (Ode::NUNITS > 1), lgl_ode_units_kernel, 3)                                                                  \
  X(K_UNITS4, LGL, (Ode::NUNITS > 1), lgl_ode_units_kernel, 4)                                                                  \
  /* mesh error (mesh_kernels.h); trajectory table: right-hand side at every node, evaluation at query times (interp_kernels.h) */ \
  X(K_MESH_YVEC, LGL, true, mesh_yvec_kernel)                                                                                   \
  X(K_MESH_ERROR, NONE, true, mesh_error_kernel, 0)                                                                             \
  X(K_INTERP_XDOT, LGL, true, interp_xdot_kernel)                                                                               \
  X(K_INTERP_EVAL, LGL, true, interp_eval_kernel)                                                                               \
  /* integrator-based mesh error (integ_kernels.h): every node interval integrated again, the per-block estimate */             \
  X(K_INTEG_STEP, LGL, true, integ_reintegrate_kernel)                                                                          \
  X(K_INTEG_ERROR, NONE, true, integ_mesh_error_kernel, 0)                                                                      \
  /* plain functions and bundles of them (func_kernels.h) */                                                                    \
  X(K_FUNC0, FUNC, true, func_kernel, 0, false)                                                                                 \
  X(K_FUNC1, FUNC, true, func_kernel, 1, false)                                                                                 \
  X(K_FUNC1_ASM, FUNC, true, func_kernel, 1, true)                                                                              \
  X(K_FUNC2, FUNC, true, func_kernel, 2, false)                                                                                 \
  X(K_FUNC2_ASM, FUNC, true, func_kernel, 2, true)                                                                              \
  X(K_BUNDLE0, BUNDLE, true, func_bundle_kernel, 0)                                                                             \
  X(K_BUNDLE1, BUNDLE, true, func_bundle_kernel, 1)                                                                             \
  X(K_BUNDLE2, BUNDLE, true, func_bundle_kernel, 2)                                                                             \
  /* batched propagation (propagate_kernels.h): end states and samples, state + STM columns, the STM's assembly */               \
  X(K_PROP_BATCH, ODE, prop_home(SCH, BLOCKED), prop_batch_kernel)                                                              \
  X(K_PROP_STM, ODE, prop_home(SCH, BLOCKED), prop_stm_kernel)                                                                  \
  X(K_PROP_JAC, ODE, prop_home(SCH, BLOCKED), prop_stm_jac_kernel)                                                               \
  /* propagation with events (propagate_event_kernels.h): the ODE's functor and the event functor in one run-time module */      \
  X(K_PROP_EVENT, ODEEV, true, prop_event_kernel)                                                                               \
  /* propagation with a controller (propagate_ctrl_kernels.h): the ODE's functor and the law's in one run-time module */         \
  X(K_PROP_CTRL_BATCH, ODECTL, true, prop_ctrl_batch_kernel)                                                                     \
  X(K_PROP_CTRL_STM, ODECTL, true, prop_ctrl_stm_kernel)                                                                         \
  X(K_PROP_CTRL_JAC, ODECTL, true, prop_ctrl_jac_kernel)                                                                         \
  /* propagation with events and the STM (propagate_event_stm_kernels.h): a run-time module of its own kind */                  \
  X(K_PROP_EVENT_STM, ODEEVS, true, prop_event_stm_kernel)                                                                       \
  X(K_PROP_EVENT_JAC, ODEEVS, true, prop_event_jac_kernel)

#define ASSET_X_ENUM(NAME, ...) NAME,
enum KSlot : int { ASSET_KERNELS(ASSET_X_ENUM) K_COUNT };
#undef ASSET_X_ENUM
#define ASSET_X_NAME(NAME, ...) #NAME,
inline const char* kslot_name(int slot) {
  static const char* const names[K_COUNT] = {ASSET_KERNELS(ASSET_X_NAME)};
  return slot >= 0 && slot < K_COUNT ? names[slot] : nullptr;
}
#undef ASSET_X_NAME

struct KernelTable {
  long long meta[MF_COUNT] = {};
  KRef k[K_COUNT];
};

struct KernelEntry {
  const char* ode;
  int xv, uv, pv;
  int mode;     // ASSET_HIP_* transcription mode
  int blocked;
  int ir, orr, nkkt;
  int kl, kstride;        // layout of the KKT blocks the kernels write (defect_dims.h: Dims::KL) and the block stride in doubles
  int seg_per_group;      // segments whose ODE results one workgroup keeps in its workspace at a time
  size_t lds_bytes;
  size_t work_doubles;    // workspace doubles per segment (ODE result slot)
  int naconst;            // plain functions: constants per application the function reads (vf.ApplConst)
  const KernelTable* table;
  KernelEntry* next;
};
inline void entry_from_table(KernelEntry& e, const char* name, const KernelTable* t) {
  const long long* m = t->meta;
  e.ode = name, e.xv = int(m[MF_XV]), e.uv = int(m[MF_UV]), e.pv = int(m[MF_PV]), e.mode = int(m[MF_MODE]);
  e.blocked = int(m[MF_BLOCKED]), e.ir = int(m[MF_IR]), e.orr = int(m[MF_OR]), e.nkkt = int(m[MF_NKKT]);
  e.kl = int(m[MF_KL]), e.kstride = m[MF_KSTRIDE] > 0 ? int(m[MF_KSTRIDE]) : e.nkkt;   // (plain functions, bundles: the reference's order)
  e.seg_per_group = int(m[MF_G]), e.lds_bytes = size_t(m[MF_LDS_BYTES]), e.work_doubles = size_t(m[MF_WORK_DOUBLES]);
  e.naconst = int(m[MF_NACONST]), e.table = t, e.next = nullptr;
}

#if defined(ASSET_PLUGIN)
// A plugin (one translation unit compiled by hipcc at run time: asset_asrl_amd/jit.py with ASSET_HIP_JIT=hipcc) collects
// its entries in a list of its own and exports it through asset_hip_plugin_entries(); asset_hip_load_plugin() splices it
// into the registry of libasset_hip.so.  Nothing here touches the host library's symbols, so the plugin needs no link
// against it.
namespace {
KernelEntry* g_plugin_head = nullptr;
}
struct Registrar {
  explicit Registrar(KernelEntry* e) {
    e->next = g_plugin_head;
    g_plugin_head = e;
  }
};
#define ASSET_PLUGIN_EXPORT()                                                                            \
  extern "C" __attribute__((visibility("default"))) ::asset_hip::KernelEntry* asset_hip_plugin_entries() { \
    return ::asset_hip::g_plugin_head;                                                                   \
  }
#else
inline KernelEntry*& registry_head() {
  static KernelEntry* head = nullptr;
  return head;
}
struct Registrar {
  explicit Registrar(KernelEntry* e) {
    e->next = registry_head();
    registry_head() = e;
  }
};
#endif

// ---- dispatch knobs of the measurement scripts (tools/README.md) -----------------------------------------------------------
// Read ONCE, and only when the process opts in with ASSET_HIP_TUNING=1, so that a stray variable in a production environment
// cannot change which kernels run.  With the opt-in, every knob that takes effect is reported on stderr; without it, a knob that
// is set is reported as ignored, so that a measurement script which forgot the opt-in does not quote the default path under the
// knob's name.  The planner takes a Tuning as an argument: Tuning() is the default dispatch whatever the environment holds.
struct Tuning {
  bool no_resident = false;   // ASSET_HIP_NO_RESIDENT: no resident kernel (nor its dense part behind the unit kernels)
  bool skip_dense = false;    // ASSET_HIP_SKIP_DENSE: the ODE stage alone (times it; the outputs are not written)
  bool no_alt_form = false;   // ASSET_HIP_NO_ALT_FORM: shapes with both dense forms (ResDims::RD_ALT) keep their tile form
  bool no_affine = false;     // ASSET_HIP_NO_AFFINE: index tables are loaded even where their rows are runs (capi.hip)
  int resident_grid = 0;      // ASSET_HIP_RESIDENT_GRID: waves of the resident kernel, level 2 (0: what the device holds)
  int grid_b = 0;             // ASSET_HIP_GRID_B: workgroups of the dense stage (0: what the LDS lets be resident)
  int alt_min = 5;            // ASSET_HIP_ALT_MIN: HALF segments per workgroup from which the one-group kernel takes the row-wise form
  int lpair_min = 1;          // ASSET_HIP_LPAIR_MIN: groups per wave from which a looped mesh takes the pair form
};
inline const Tuning& tuning() {
  static const Tuning tn = [] {
    Tuning r;
    const char* on = std::getenv("ASSET_HIP_TUNING");
    const bool opted = on && std::atoi(on) != 0;
    bool warned = false;
    auto knob = [&](const char* name) -> const char* {
      const char* v = std::getenv(name);
      if (v && opted) std::fprintf(stderr, "asset_hip: tuning knob %s=%s is in effect (ASSET_HIP_TUNING=1)\n", name, v);
      if (v && !opted && !warned) {
        warned = true;
        std::fprintf(stderr, "asset_hip: %s is set but IGNORED (dispatch knobs need ASSET_HIP_TUNING=1)\n", name);
      }
      return opted ? v : nullptr;
    };
    r.no_resident = knob("ASSET_HIP_NO_RESIDENT") != nullptr;
    r.skip_dense = knob("ASSET_HIP_SKIP_DENSE") != nullptr;
    r.no_alt_form = knob("ASSET_HIP_NO_ALT_FORM") != nullptr;
    r.no_affine = knob("ASSET_HIP_NO_AFFINE") != nullptr;
    if (const char* v = knob("ASSET_HIP_RESIDENT_GRID")) r.resident_grid = std::atoi(v);
    if (const char* v = knob("ASSET_HIP_GRID_B")) r.grid_b = std::atoi(v);
    if (const char* v = knob("ASSET_HIP_ALT_MIN")) r.alt_min = std::atoi(v);
    if (const char* v = knob("ASSET_HIP_LPAIR_MIN")) r.lpair_min = std::atoi(v);
    return r;
  }();
  return tn;
}

// ---- the launch plan of one evaluation ------------------------------------------------------------------------------------------
// plan_lgl decides (no HIP call, no environment, no allocation); launch_plan walks what it decided.
struct PlanRequest {
  int level;          // derivatives: 0 value, 1 + Jacobian, 2 + adjoint Hessian
  bool blocks;        // KKT blocks are written
  bool asmb;          // KKT entries are added straight into the solver's value array (EvalArgs::kmap)
  bool adjgrad;       // the adjoint gradient is wanted and multipliers are given (AGX && L)
  bool res_record;    // the handle holds the lane record of the resident kernel (EvalArgs::lane_consts_res)
};
enum PlanExtra { PLAN_NO_EXTRA = 0, PLAN_GP = 1, PLAN_WORK_RO = 2 };   // second kernel argument: none, segments per group, the workspace read-only
struct PlanStep {
  int slot;
  unsigned grid_x, grid_y, block;
  size_t lds_bytes;
  int extra, gp;
};
struct LaunchPlan {
  int nsteps = 0;
  int units_gp = 0;   // EvalArgs::units_gp of the last step: the dense part follows the XCD placement of the unit stage
  PlanStep step[3];
};

// ODE stage by units: segments per group so that the launch is about one workgroup per SIMD (groups x waves_per_seg ~ 4 per CU)
inline int units_group(int nseg, int waves_per_seg, int cs, int cus) {
  const int gp = int(((long long)nseg * waves_per_seg + 4 * cus - 1) / (4 * cus)), gpmax = 64 / cs;
  return gp < 1 ? 1 : (gp > gpmax ? gpmax : gp);
}
// heavy ODEs, level 2: the one-launch unit stage while its workgroups are at most this many rounds of the device's SIMDs -- beyond
// every mesh in practice, because it measured faster at every size tried (Betts-LGL5 x 1 000: 30.3 against 41.5 us, x 10 000:
// 191.7 / 200.0; Betts-LGL7 x 5 000: 145.1 / 151.1); two launches (interior units, then cardinal units) beyond
constexpr int kUnitsOneLaunchRounds = 1000;

inline hipError_t plan_lgl(const KernelTable& t, const PlanRequest& rq, int nseg, int cus, const Tuning& tn, LaunchPlan& p) {
  const long long* m = t.meta;
  const int level = rq.level;
  const bool asmb = rq.asmb;
  p = LaunchPlan();
  if (level < 0 || level > 2 || nseg < 1 || cus < 1) return hipErrorInvalidValue;
  auto add = [&](int slot, long long gx, long long gy, int block, long long lds, int extra = PLAN_NO_EXTRA, int gp = 0) {
    p.step[p.nsteps++] = PlanStep{slot, unsigned(gx), unsigned(gy), unsigned(block), size_t(lds), extra, gp};
  };
  auto by = [&](int l1, int l1a, int l2, int l2a) { return level == 2 ? (asmb ? l2a : l2) : (asmb ? l1a : l1); };
  auto ceil_div = [](long long a, long long b) { return (a + b - 1) / b; };
  auto least = [](long long a, long long b) { return a < b ? a : b; };

  // value (evalOCC), and value + J^T lam without a Jacobian (evalRHS): one launch of the vector-Jacobian kernel, for the value
  // without its gradient parts (a table without K_VALUE has no value-only kind: the launch reports the missing kernel)
  if (level == 0 || (level == 1 && !rq.blocks && !asmb && rq.adjgrad && t.k[K_ADJGRAD])) {
    add(level == 0 ? K_VALUE : K_ADJGRAD, ceil_div(nseg, m[MF_ADJ_GP]), 1, 64, m[MF_ADJ_LDS_BYTES]);
    return hipSuccess;
  }

  // resident kernel (defect_resident.h): the ODE results stay in LDS.  One group per wave while a wave's share is at most GR
  // segments, the looped instantiation beyond.
  const int waves_dev = cus * 4 * int(m[MF_RES_WPS]);
  if (m[MF_RES_GR] > 0 && !tn.no_resident && !tn.skip_dense && rq.res_record && t.k[by(K_RES1, K_RES1_ASM, K_RES2, K_RES2_ASM)] &&
      (!asmb || m[MF_RES_ASM])) {
    const int waves = (level == 2 && tn.resident_grid > 0) ? tn.resident_grid : waves_dev;
    const long long share = ceil_div(nseg, waves);
    const bool one = share <= m[MF_RES_GR];
    const int kr = one ? by(K_RES1, K_RES1_ASM, K_RES2, K_RES2_ASM) : by(K_RESL1, K_RESL1_ASM, K_RESL2, K_RESL2_ASM);
    if (t.k[kr]) {
      // two-wave workgroups (a region of LDS each): the one-group kernel of a pair shape -- and, on every looped mesh, the looped
      // level-2 block kernel of the shapes that are built with one (ResDims::LOOP_PAIR: row-wise dense part, a right-hand side
      // heavy enough for the shared ODE stage to pay for the pair's barriers -- profiles/r6_forms2.txt)
      const bool lpair = level == 2 && !one && !asmb && m[MF_RES_LOOP_NWV] > 1 && t.k[K_RESLP] && !(tn.no_alt_form && m[MF_RES_ALT]) &&
                         share >= tn.lpair_min * m[MF_RES_GR];
      const int nwv = ((one && m[MF_RES_NWV] > 1) || lpair) ? 2 : 1;
      const long long nwg = ceil_div(least(nseg, waves), nwv);
      // shapes with both forms of the dense part (ResDims::RD_ALT): rows in the one-group kernel from two and a half segments per
      // workgroup on (with UNITC the row-wise part is the cheaper one wherever its passes -- four / two segments -- are not mostly
      // empty: Reentry-LGL7 x 2 500 15.8 against 16.1 us, x 5 000 20.5 / 20.9, x 10 000 26.4 / 28.4; x 1 000 13.8 / 13.2), tiles below
      const bool alt = level == 2 && one && nwv == 2 && !asmb && !tn.no_alt_form && m[MF_RES_ALT] && t.k[K_RES_ALT] &&
                       2LL * nseg >= tn.alt_min * nwg;
      add(lpair ? K_RESLP : (alt ? K_RES_ALT : kr), nwg, 1, 64 * nwv, m[MF_RES_LDS_BYTES] / (m[MF_RES_NWV] > 1 ? 2 : 1) * nwv);
      return hipSuccess;
    }
  }

  // dense launch: persistent single-wave workgroups, as many as the LDS lets be resident
  // (an even number of waves per CU spreads evenly over the 4 SIMDs; 7 per CU measured 30% slower than 6)
  const int fit_b = int((160 * 1024) / m[MF_BYTES_DENSE]);
  const int per_cu_b = fit_b < 1 ? 1 : (fit_b >= 8 ? 8 : (fit_b >= 6 ? 6 : (fit_b >= 4 ? 4 : fit_b)));
  const long long grid_b = least(nseg, tn.grid_b > 0 ? tn.grid_b : cus * per_cu_b);

  if (m[MF_FUSED] && !tn.skip_dense) {
    // STAGE 4: two-wave workgroups, the ODE bodies are issued once per pair of waves
    // (measured, 10 000 segments: TwoBody-LGL5-BlockConstant 42.2 -> 39.6 us, Reentry-LGL7 43.2 -> 43.0 us; with 2-3 segments per
    //  wave -- Reentry-LGL7 x 5 000 -- the pair's barriers cost more than the shared bodies save: 29.6 -> 32.9 us, so short shares
    //  keep the one-wave form)
    const long long pairs = grid_b / 2, share2 = pairs > 0 ? ceil_div(nseg, 2 * pairs) : 0;
    if (level == 2 && m[MF_FUSED2] && !asmb && pairs > 0 && share2 >= 4 && share2 <= m[MF_GF2] / 2) {
      add(K_LGL2_S4, pairs, 1, 128, m[MF_BYTES_FUSED2]);
      return hipSuccess;
    }
    // STAGE 3: a single launch when every workgroup's share fits one group of the fused kernel (also with on-device assembly: the
    // dense part places its entries through the map either way)
    const int k3 = by(K_LGL1_S3, K_LGL1_S3_ASM, K_LGL2_S3, K_LGL2_S3_ASM);
    if (ceil_div(nseg, grid_b) <= m[MF_GF] && t.k[k3]) {
      add(k3, grid_b, 1, 64, m[MF_BYTES_DENSE]);
      return hipSuccess;
    }
  }

  // ---- two stages: the ODE results go through the workspace
  const int nunits = int(m[MF_NUNITS]), cs = int(m[MF_CS]);
  int xcd_gp = 0;   // segments per group of a unit stage placed by XCD (below)
  if (nunits > 1 && level == 1 && t.k[K_UNITSJ] && (long long)nseg * cs <= 64LL * cus) {
    // heavy right-hand side, Jacobian kinds: one wave per output unit (defect_units.h, PHASE 3) -- while the mesh leaves SIMDs
    // idle: the units recompute what they share, and from ~16 cardinal points per SIMD on the one-body-per-lane stage is the
    // faster one (Betts-LGL5: 1 000 segments 21.5 against 48.1 us, 5 000: 48.8 / 53.8, 10 000: 85.0 / 72.7)
    const int gp = units_group(nseg, nunits, cs, cus);
    add(K_UNITSJ, ceil_div(nseg, gp), nunits, 64, m[MF_UNITS_BASE_BYTES] + gp * m[MF_UNITS_SLOT_BYTES], PLAN_GP, gp);
  } else if (nunits > 1 && level == 2) {
    // One launch (PHASE 4: every cardinal unit forms the interior gradients it needs itself, so 2 x units waves per segment)
    const int gp4 = units_group(nseg, 2 * nunits, cs, cus);
    const long long ng4 = ceil_div(nseg, gp4);
    if (t.k[K_UNITS4] && ng4 * 2 * nunits <= (long long)kUnitsOneLaunchRounds * 4 * cus) {
      // XCD-aware placement (MI355X: 8 XCDs; on a part with another count the mapping below is still a valid split of the work --
      // it only stops coinciding with the L2s): workgroups go to the eight XCDs round robin in launch order (x fastest), so with
      // the number of groups padded to a multiple of eight every unit of group g runs on XCD g % 8 -- its slot is assembled in ONE
      // L2 (no 32-byte sector written back half-filled by several of them) -- and the dense part reads it there
      add(K_UNITS4, (ng4 + 7) & ~7LL, 2 * nunits, 64, m[MF_UNITS_BASE_BYTES] + gp4 * m[MF_UNITS_SLOT_BYTES], PLAN_GP, gp4);
      // (the dense part follows only while its shares stay as even as the plain split's -- every group is divided among a whole
      //  number of waves: Betts-LGL5 x 1 000: 29.9 -> 28.6 us; x 2 000, where that leaves 3 segments to some waves and 2 to others:
      //  51.3 -> 55.7 us.  The padded unit grid alone: Betts-LGL5 x 5 000 106.7 -> 101.2 us, Betts-LGL7 x 5 000 145.4 -> 138.0 us)
      const long long gx = (ng4 + 7) / 8, wpg = gx > 0 ? (waves_dev / 8) / gx : 0;
      if (waves_dev % 8 == 0 && wpg > 0 && ceil_div(gp4, wpg) <= ceil_div(nseg, waves_dev)) xcd_gp = gp4;
    } else {
      const int gp = units_group(nseg, nunits, cs, cus);
      const long long bytes = m[MF_UNITS_BASE_BYTES] + gp * m[MF_UNITS_SLOT_BYTES];
      add(K_UNITS0, ceil_div(nseg, gp), nunits, 64, bytes, PLAN_GP, gp);
      add(K_UNITS1, ceil_div(nseg, gp), nunits, 64, bytes, PLAN_GP, gp);
    }
  } else {
    // the three ODE phases are latency chains, so spread the segments over every resident wave (fewest passes per wave); a
    // workgroup walks its share in groups of at most G segments (= 64 points of the widest phase)
    const int fit_a = int((160 * 1024) / m[MF_BYTES_ODE]);
    const int per_cu_a = fit_a < 1 ? 1 : (fit_a >= 8 ? 8 : (fit_a >= 4 ? 4 : fit_a));
    add(level == 2 ? K_LGL2_S1 : K_LGL1_S1, least(nseg, cus * per_cu_a), 1, 64, m[MF_BYTES_ODE]);
  }
  if (tn.skip_dense) return hipSuccess;
  p.units_gp = xcd_gp;

  if (level == 2 && m[MF_RESD_GR] > 0 && !tn.no_resident && rq.res_record && t.k[asmb ? K_RESD_ASM : K_RESD]) {
    // dense part of the resident kernel over the slots the units wrote (XCD-aware placement: the whole grid, a wave's segments
    // follow from its XCD; otherwise a wave per segment at most)
    add(asmb ? K_RESD_ASM : K_RESD, xcd_gp > 0 ? waves_dev : least(nseg, waves_dev), 1, 64, m[MF_RES_LDS_BYTES]);
  } else if (m[MF_WIDE] && !asmb && m[MF_ROWS_LDS_BYTES] > 0 && cs >= 3 && t.k[level == 2 ? K_ROWS2 : K_ROWS1]) {
    // (LGL3: two nodes, IR = 2 q -- one of the two H blocks nearly empty: 487 against 399 us for 12 500 32-state segments; kept
    //  with the tile kernel)
    add(level == 2 ? K_ROWS2 : K_ROWS1, least(nseg, cus), 1, 256, m[MF_ROWS_LDS_BYTES], PLAN_WORK_RO);
  } else if (m[MF_WIDE]) {   // one four-wave workgroup per CU, or MF_WIDE_WGS of them (defect_wide.h)
    add(by(K_WIDE1, K_WIDE1_ASM, K_WIDE2, K_WIDE2_ASM), least(nseg, cus * m[MF_WIDE_WGS]), 1, 256, m[MF_BYTES_DENSE]);
  } else {
    add(by(K_LGL1_S2, K_LGL1_S2_ASM, K_LGL2_S2, K_LGL2_S2_ASM), grid_b, 1, 64, m[MF_BYTES_DENSE]);
  }
  return hipSuccess;
}

// Every kernel that takes the arguments of an evaluation has the one parameter list of eval_args.h, and this is the one place that
// fills it: the values through eval_args_pack -- with the workgroups the launch is made with -- then the kernel's own trailing parameter.
inline hipError_t launch_eval(const KRef& k, dim3 grid, dim3 block, size_t shmem, hipStream_t st, const EvalArgs& a, void* extra = nullptr) {
  EvalKernArgs ka;
  void* kargs[kEvalParams + 1];
  eval_args_pack(a, grid.x, ka, kargs);
  kargs[kEvalParams] = extra;      // (kernels without a trailing parameter never read it)
  return klaunch(k, grid, block, shmem, st, kargs);
}

inline hipError_t launch_plan(const KernelTable& t, const LaunchPlan& p, const EvalArgs& a, hipStream_t st) {
  EvalArgs args = a;
  for (int i = 0; i < p.nsteps; i++) {
    const PlanStep& s = p.step[i];
    if (i + 1 == p.nsteps && p.units_gp > 0) args.units_gp = p.units_gp;
    int gp = s.gp;
    const double* work_ro = a.work;
    void* const extra = s.extra == PLAN_GP ? static_cast<void*>(&gp) : static_cast<void*>(&work_ro);
    const hipError_t e = launch_eval(t.k[s.slot], dim3(s.grid_x, s.grid_y), dim3(s.block), s.lds_bytes, st, args, extra);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
inline PlanRequest plan_request(int level, const EvalArgs& a) {
  return PlanRequest{level, a.KKT != nullptr, a.kmap != nullptr, a.AGX && a.L, a.lane_consts_res != nullptr};
}

// A plain function batched over applications: transcription id 0 (func_kernels.h).  plan_func decides (no HIP call): the kernel
// slot, the grid, the dynamic LDS and the applications per workgroup -- the block kinds of a function with FuncStage::APW > 0 take
// APW applications per workgroup and stage their blocks in LDS, everything else takes 64 and no LDS.  The launcher, the bundle
// launcher (capi.hip) and asset_hip_defect_launch_plan all read it.
struct FuncPlan {
  int slot;
  unsigned grid;
  size_t lds_bytes;
  int apw;
};
inline FuncPlan plan_func(const long long* meta, int level, bool assembled, int nseg) {
  const bool asmb = level >= 1 && assembled;
  const bool staged = level >= 1 && !asmb && meta[MF_G] > 0;
  const int apw = staged ? int(meta[MF_G]) : 64;
  const int slot = level == 0 ? K_FUNC0 : (level == 1 ? (asmb ? K_FUNC1_ASM : K_FUNC1) : (asmb ? K_FUNC2_ASM : K_FUNC2));
  return FuncPlan{slot, unsigned((nseg + apw - 1) / apw), staged ? size_t(meta[MF_LDS_BYTES]) : 0, apw};
}
inline hipError_t launch_func_table(const KernelTable& t, int level, const EvalArgs& a, hipStream_t st) {
  if (level < 0 || level > 2) return hipErrorInvalidValue;
  const FuncPlan p = plan_func(t.meta, level, a.kmap != nullptr, a.nseg);
  return launch_eval(t.k[p.slot], dim3(p.grid), dim3(64), p.lds_bytes, st, a);
}

inline hipError_t entry_launch(const KernelEntry* ke, int level, const EvalArgs& a, int cus, hipStream_t st) {
  if (ke->table->meta[MF_KIND] == 2) return launch_func_table(*ke->table, level, a, st);
  LaunchPlan p;
  const hipError_t e = plan_lgl(*ke->table, plan_request(level, a), a.nseg, cus, tuning(), p);
  return e != hipSuccess ? e : launch_plan(*ke->table, p, a, st);
}

// de Boor mesh-error estimate (mesh_kernels.h); only transcriptions of an ODE have it
inline bool entry_has_mesh(const KernelEntry* ke) { return bool(ke->table->k[K_MESH_YVEC]); }
inline hipError_t entry_mesh(const KernelEntry* ke, const MeshArgs& a, hipStream_t st) {
  const MeshScheme sc = mesh_scheme(ke->mode);
  MeshArgs args = a;
  const int grid = (a.nb + 63) / 64;
  void* yargs[] = {&args};
  hipError_t e = klaunch(ke->table->k[K_MESH_YVEC], dim3(grid), dim3(64), 0, st, yargs);
  if (e != hipSuccess) return e;
  int xv = ke->xv;
  double order = sc.order, weight = sc.error_weight;
  void* eargs[] = {&args, &xv, &order, &weight};
  return klaunch(ke->table->k[K_MESH_ERROR], dim3(grid), dim3(64), 0, st, eargs);
}

// integrator-based mesh-error estimate (integ_kernels.h); only transcriptions of an ODE have it.  `a.max_err` is zeroed here: the
// lanes of stage 1 raise it
inline bool entry_has_integ(const KernelEntry* ke) { return bool(ke->table->k[K_INTEG_STEP]) && bool(ke->table->k[K_INTEG_ERROR]); }
inline hipError_t entry_integ(const KernelEntry* ke, const IntegArgs& a, hipStream_t st) {
  IntegArgs args = a;
  const int K = interp_basis(ke->mode).cs - 1, lanes = integ_lanes(ke->xv);
  const long long nint = (long long)a.nb * K;
  hipError_t e = hipMemsetAsync(a.max_err, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  void* sargs[] = {&args};
  e = klaunch(ke->table->k[K_INTEG_STEP], dim3(unsigned((nint + lanes - 1) / lanes)), dim3(64), 0, st, sargs);
  if (e != hipSuccess) return e;
  int n = ke->xv, N = ke->xv + 1 + ke->uv + ke->pv, k = K;
  double order = mesh_scheme(ke->mode).order;
  void* eargs[] = {&args, &n, &N, &k, &order};
  return klaunch(ke->table->k[K_INTEG_ERROR], dim3((a.nb + 63) / 64), dim3(64), 0, st, eargs);
}

// batched propagation (propagate_kernels.h): the ODE's home entry (prop_home) has the three kernels; capi.hip launches them by the
// plan of capi/propagate_plan.h
inline bool entry_has_prop(const KernelEntry* ke) {
  return bool(ke->table->k[K_PROP_BATCH]) && bool(ke->table->k[K_PROP_STM]) && bool(ke->table->k[K_PROP_JAC]);
}

// trajectory table (interp_kernels.h); only transcriptions of an ODE have it.  entry_interp_table: stage 1 (a.traj -> a.xdot, a.tb),
// entry_interp: stage 2 (a.times -> a.out, a.dout)
inline bool entry_has_interp(const KernelEntry* ke) { return bool(ke->table->k[K_INTERP_XDOT]) && bool(ke->table->k[K_INTERP_EVAL]); }
inline hipError_t entry_interp_table(const KernelEntry* ke, const InterpArgs& a, hipStream_t st) {
  InterpArgs args = a;
  void* kargs[] = {&args};
  const long long nodes = (long long)a.nb * (interp_basis(ke->mode).cs - 1) + 1;
  return klaunch(ke->table->k[K_INTERP_XDOT], dim3(unsigned((nodes + 63) / 64)), dim3(64), 0, st, kargs);
}
inline hipError_t entry_interp(const KernelEntry* ke, const InterpArgs& a, int cus, hipStream_t st) {
  if (a.nq <= 0) return hipSuccess;
  InterpArgs args = a;
  void* kargs[] = {&args};
  // memory-bound: at most 8 workgroups per CU, each walks its share of the query groups
  const long long groups = (a.nq + INTERP_QG - 1) / INTERP_QG, cap = (long long)(cus > 0 ? cus : 256) * 8;
  return klaunch(ke->table->k[K_INTERP_EVAL], dim3(unsigned(groups < cap ? groups : cap)), dim3(256), 0, st, kargs);
}

// per-lane constants of the dense stage for derivative level 1 / 2: table size in bytes (0: none) and the kernel filling it
// (level 0 stands for the record of the resident kernel)
inline size_t entry_lane_bytes(const KernelEntry* ke, int level) {
  if (ke->table->meta[MF_KIND] != 1) return 0;
  return level >= 2 ? size_t(ke->table->meta[MF_LANE_BYTES2])
                    : (level == 1 ? size_t(ke->table->meta[MF_LANE_BYTES1]) : size_t(ke->table->meta[MF_LANE_BYTES_RES]));
}
inline hipError_t entry_lane_setup(const KernelEntry* ke, int level, void* out, hipStream_t st) {
  void* kargs[] = {&out};
  const KernelTable& t = *ke->table;
  if (level == 0) return klaunch(t.k[K_RES_SETUP], dim3(1), dim3(64), 0, st, kargs);
  return klaunch(t.meta[MF_WIDE] ? t.k[K_WIDE_SETUP] : (level >= 2 ? t.k[K_LANE_SETUP2] : t.k[K_LANE_SETUP1]), dim3(1), dim3(64), 0, st, kargs);
}

// ---- tables of the kernels linked into this translation unit ---------------------------------------------------------
#define ASSET_KPTR(...) reinterpret_cast<const void*>(&__VA_ARGS__)
#define ASSET_FILL_LGLG(NAME, COND, T, ...) if constexpr (COND) r.k[NAME].host = ASSET_KPTR(T<Ode, SCH, BLOCKED, G, ##__VA_ARGS__>);
#define ASSET_FILL_LGL(NAME, COND, T, ...) if constexpr (COND) r.k[NAME].host = ASSET_KPTR(T<Ode, SCH, BLOCKED, ##__VA_ARGS__>);
#define ASSET_FILL_NONE(NAME, COND, T, ...) if constexpr (COND) r.k[NAME].host = ASSET_KPTR(T<__VA_ARGS__>);
#define ASSET_FILL_ODE(NAME, COND, T, ...) if constexpr (COND) r.k[NAME].host = ASSET_KPTR(T<Ode, ##__VA_ARGS__>);
#define ASSET_FILL_FUNC(NAME, COND, T, ...)
#define ASSET_FILL_BUNDLE(NAME, COND, T, ...)
#define ASSET_FILL_ODEEV(NAME, COND, T, ...)
#define ASSET_FILL_ODECTL(NAME, COND, T, ...)
#define ASSET_FILL_ODEEVS(NAME, COND, T, ...)
#define ASSET_X_FILL(NAME, FAMILY, COND, T, ...) ASSET_FILL_##FAMILY(NAME, COND, T, ##__VA_ARGS__)
template <class Ode, int SCH, bool BLOCKED, int G>
const KernelTable* lgl_static_table() {
  using D = Dims<Ode, SCH, BLOCKED>;
  static KernelTable t = [] {
    KernelTable r;
    for (int i = 0; i < MF_COUNT; i++) r.meta[i] = LglMeta<Ode, SCH, BLOCKED, G>::v[i];
    ASSET_KERNELS(ASSET_X_FILL)
    return r;
  }();
  return &t;
}
#undef ASSET_FILL_LGLG
#undef ASSET_FILL_LGL
#undef ASSET_FILL_NONE
#undef ASSET_FILL_ODE
#undef ASSET_FILL_FUNC
#define ASSET_FILL_LGLG(NAME, COND, T, ...)
#define ASSET_FILL_LGL(NAME, COND, T, ...)
#define ASSET_FILL_NONE(NAME, COND, T, ...)
#define ASSET_FILL_ODE(NAME, COND, T, ...)
#define ASSET_FILL_FUNC(NAME, COND, T, ...) r.k[NAME].host = ASSET_KPTR(T<F, ##__VA_ARGS__>);
template <class F>
const KernelTable* func_static_table() {
  static KernelTable t = [] {
    KernelTable r;
    for (int i = 0; i < MF_COUNT; i++) r.meta[i] = FuncMeta<F>::v[i];
    ASSET_KERNELS(ASSET_X_FILL)
    return r;
  }();
  return &t;
}
#undef ASSET_FILL_LGLG
#undef ASSET_FILL_LGL
#undef ASSET_FILL_NONE
#undef ASSET_FILL_ODE
#undef ASSET_FILL_FUNC
#undef ASSET_FILL_BUNDLE
#undef ASSET_FILL_ODEEV
#undef ASSET_FILL_ODECTL
#undef ASSET_FILL_ODEEVS
#undef ASSET_X_FILL
#undef ASSET_KPTR

struct StaticEntry {   // (static initialisation: the table is filled and the entry registered before main)
  KernelEntry e;
  Registrar* reg;
  StaticEntry(const char* name, const KernelTable* t) {
    entry_from_table(e, name, t);
    reg = new Registrar(&e);
  }
};

#define ASSET_REGISTER_FUNC(FN) \
  static ::asset_hip::StaticEntry entry_##FN##_func(FN::name(), ::asset_hip::func_static_table<FN>());

// Trapezoidal = transcription id 1 of the same kernels (defect_dims.h: Dims::TRAP)
#define ASSET_REGISTER_TRAP(ODE, BLK, G) ASSET_REGISTER_LGL(ODE, 1, BLK, G)

#define ASSET_REGISTER_LGL(ODE, CSV, BLK, G) \
  static ::asset_hip::StaticEntry entry_##ODE##_##CSV##_##BLK(ODE::name(), ::asset_hip::lgl_static_table<ODE, CSV, (BLK != 0), G>());

// ---- name expressions of the kernels of a run-time module (capi.hip: asset_hip_jit_plugin) -----------------------------
// kind 1: `type` is the ODE functor, kind 2: the function functor, kind 3: the comma-separated functor list of a bundle, kind 4: "Ode, Ev",
// the ODE functor and the event functor of a propagation with events, kind 5: "Ode, Ctl", the ODE functor and its control law, kind 6: "Ode, Ev"
// again, for the propagation with events and the STM.  Slots
// without a kernel for that kind: empty string.
inline std::string rtc_kernel_expr(int slot, int kind, const std::string& type, int csv, bool blocked, int g) {
  const std::string none, lgl = type + ", " + std::to_string(csv) + ", " + (blocked ? "true" : "false"), lglg = lgl + ", " + std::to_string(g);
  // (module kind that has the slot, what the family puts before the trailing arguments -- a bundle: after them)
  auto expr = [&](const char* tmpl, std::string trailing, int slot_kind, const std::string& lead, bool lead_last = false) {
    if (slot_kind != kind) return std::string();
    const std::string a = lead_last ? trailing : lead, b = lead_last ? lead : trailing;
    return "asset_hip::" + std::string(tmpl) + "<" + a + (a.empty() || b.empty() ? "" : ", ") + b + ">";
  };
#define ASSET_RTC_LGLG 1, lglg
#define ASSET_RTC_LGL 1, lgl
#define ASSET_RTC_NONE 1, none
#define ASSET_RTC_ODE (prop_home(csv, blocked) ? 1 : 0), type
#define ASSET_RTC_FUNC 2, type
#define ASSET_RTC_BUNDLE 3, type, true
#define ASSET_RTC_ODEEV 4, type
#define ASSET_RTC_ODECTL 5, type
#define ASSET_RTC_ODEEVS 6, type
#define ASSET_X_EXPR(NAME, FAMILY, COND, T, ...) case NAME: return expr(#T, #__VA_ARGS__, ASSET_RTC_##FAMILY);
  switch (slot) { ASSET_KERNELS(ASSET_X_EXPR) }
#undef ASSET_X_EXPR
#undef ASSET_RTC_LGLG
#undef ASSET_RTC_LGL
#undef ASSET_RTC_NONE
#undef ASSET_RTC_ODE
#undef ASSET_RTC_FUNC
#undef ASSET_RTC_BUNDLE
#undef ASSET_RTC_ODEEV
#undef ASSET_RTC_ODECTL
#undef ASSET_RTC_ODEEVS
  return "";
}

}  // namespace asset_hip

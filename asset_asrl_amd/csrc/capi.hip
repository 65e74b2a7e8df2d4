// C ABI of libasset_hip.so (see include/asset_hip.h for the contract and the reference interfaces replaced).
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <memory>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <algorithm>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/asset_hip.h"
#include <dlfcn.h>
#include <unistd.h>

#include "registry.h"

namespace asset_hip {
// values[loc[l]] = sum of stage[ptr[l] .. ptr[l+1]) in a FIXED order: thread t of the block adds cells t, t+256, ... in
// sequence, then the 256 partial sums are folded by a tree of fixed shape.  One block per location.
__global__ __launch_bounds__(256) void asm_reduce_kernel(double* values, const double* stage, const int* ptr, const int* loc) {
  __shared__ double part[256];
  const int l = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int k = ptr[l] + t; k < ptr[l + 1]; k += 256) s += stage[k];
  part[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) values[loc[l]] = part[0];
}

// RHS fill on the device (NonLinearProgram.h:401-407 RHSFillOP: target[rows[k]] += coeffs[k]) as a GATHER: one thread per
// target row adds that row's contributions (ptr / src: CSR by row over the block entries, source order) in a fixed
// order -- no atomics, bitwise repeatable.  Rows with many contributors (phase parameters) take gather_long_kernel.
__global__ __launch_bounds__(256) void rhs_gather_kernel(double* target, const double* blocks, const int* rows, const int* ptr,
                                                         const int* src, int nrows, int long_from) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows || r >= long_from) return;
  double s = 0.0;
  for (int k = ptr[r]; k < ptr[r + 1]; k++) s += blocks[src[k]];
  target[rows[r]] += s;
}
__global__ __launch_bounds__(256) void rhs_gather_long_kernel(double* target, const double* blocks, const int* rows,
                                                              const int* ptr, const int* src, int long_from) {
  __shared__ double part[256];
  const int r = long_from + blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  for (int k = ptr[r] + t; k < ptr[r + 1]; k += 256) s += blocks[src[k]];
  part[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) target[rows[r]] += part[0];
}

}  // namespace asset_hip

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hipfail(hipError_t e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
  return int(e) > 0 ? int(e) : ASSET_HIP_ENODEV;
}
#define HIP_TRY(expr)                                     \
  do {                                                    \
    hipError_t _e = (expr);                               \
    if (_e != hipSuccess) return hipfail(_e, #expr);      \
  } while (0)

const asset_hip::KernelEntry* find_entry(const char* ode, int mode, int blocked) {
  for (auto* e = asset_hip::registry_head(); e; e = e->next)
    if (!std::strcmp(e->ode, ode) && e->mode == mode && e->blocked == (blocked ? 1 : 0)) return e;
  return nullptr;
}

int level_of(int what) {
  switch (what & 0xff) {
    case ASSET_HIP_CON: return 0;
    case ASSET_HIP_CON_ADJGRAD:
    case ASSET_HIP_JAC:
    case ASSET_HIP_JAC_ADJGRAD: return 1;
    case ASSET_HIP_JAC_ADJGRAD_HESS: return 2;
  }
  return -1;
}

}  // namespace

struct asset_hip_defect {
  const asset_hip::KernelEntry* ke = nullptr;
  int nseg = 0, n_primal = 0, n_equal = 0, device = 0;
  int cus = 256;
  // what the buffers below were sized for (asset_hip_defect_rebind keeps them while the new mesh fits)
  int cap_seg = 0, cap_primal = 0, cap_equal = 0;
  int* d_vindex = nullptr;
  int* d_cindex = nullptr;
  // staging for the host-pointer entry point (allocated lazily)
  double *d_X = nullptr, *d_L = nullptr, *d_fx = nullptr, *d_agx = nullptr, *d_kkt = nullptr;
  double* d_work = nullptr;  // per-workgroup ODE result slots
  void* d_lane[3] = {nullptr, nullptr, nullptr};   // per-lane constants of the dense stage by derivative level
  double* d_aconst = nullptr;      // constants of every application of a plain function (asset_hip_defect_set_appl_consts)
  // on-device KKT assembly (asset_hip_defect_set_kkt_map)
  int32_t* d_map = nullptr;        // value location of every accumulator entry, fragment order (defect_kernels.h, ASM)
  size_t map_len = 0;
  double* d_values = nullptr;      // [value_hi - value_lo) staging for the host-pointer entry point
  double* h_values = nullptr;      // pinned mirror of d_values
  long long value_lo = 0, value_hi = 0, nvalues = 0;
  // locations with three or more contributing slots: staged cells + fixed-order reduction (defect_dims.h, asm_reduce_kernel)
  double* d_stage = nullptr;
  int *d_multi_ptr = nullptr, *d_multi_loc = nullptr;
  int nmulti = 0;
  size_t nstage = 0;
  // device RHS fill (asset_hip_defect_eval_kkt_device): CSR by target row over the FX / AGX block entries
  int *d_fx_rows = nullptr, *d_fx_ptr = nullptr, *d_fx_src = nullptr, *d_gx_rows = nullptr, *d_gx_ptr = nullptr, *d_gx_src = nullptr;
  int n_fx_rows = 0, fx_long_from = 0, n_gx_rows = 0, gx_long_from = 0;
  bool rhs_tables_ready = false;
  int affine = 0, aff_v0 = 0, aff_vs = 0, aff_c0 = 0, aff_cs = 0;   // index rows that are runs (EvalArgs::affine)
  int bundles = 0;                   // bundles that hold this handle (asset_hip_bundle_create)
  bool destroy_pending = false;      // asset_hip_defect_destroy was called while a bundle held it: freed with the last bundle
  double *d_fxb = nullptr, *d_agxb = nullptr;    // block buffers of that entry point
  std::vector<int32_t> h_vindex, h_cindex;       // kept for the RHS tables (built on first use)
  hipStream_t stream = nullptr;
  // the caller's stream of the last *_device entry point (asset_hip_defect_rebind drains it before it touches the tables those
  // launches read: a torch side stream or hipStreamLegacy is not ordered with the handle's own stream)
  hipStream_t last_stream = nullptr;
  bool last_stream_used = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

extern "C" {

const char* asset_hip_last_error(void) { return g_err.c_str(); }
// (for the other translation units of the library -- capi_sharded.hip; not part of the public interface)
__attribute__((visibility("hidden"))) void asset_hip_set_last_error(const char* msg) { g_err = msg ? msg : ""; }
const char* asset_hip_version(void) { return "asset_hip 0.1 (gfx950)"; }

int asset_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int asset_hip_num_odes(void) {
  int n = 0;
  for (auto* e = asset_hip::registry_head(); e; e = e->next) {
    bool first = true;
    for (auto* f = e->next; f; f = f->next)
      if (!std::strcmp(f->ode, e->ode)) first = false;
    n += first;
  }
  return n;
}

const char* asset_hip_ode_name(int i) {
  int n = 0;
  for (auto* e = asset_hip::registry_head(); e; e = e->next) {
    bool first = true;
    for (auto* f = e->next; f; f = f->next)
      if (!std::strcmp(f->ode, e->ode)) first = false;
    if (first && n++ == i) return e->ode;
  }
  return nullptr;
}

int asset_hip_ode_sizes(const char* ode, int* xv, int* uv, int* pv) {
  if (!ode) return fail(ASSET_HIP_EINVAL, "null ode name");
  for (auto* e = asset_hip::registry_head(); e; e = e->next)
    if (!std::strcmp(e->ode, ode)) {
      if (xv) *xv = e->xv;
      if (uv) *uv = e->uv;
      if (pv) *pv = e->pv;
      return 0;
    }
  return fail(ASSET_HIP_ENOODE, std::string("unknown ODE '") + ode + "'");
}


// ---- in-process run-time compilation (hiprtc) ---------------------------------------------------------------------------
namespace {
// what one compilation leaves behind: the code object and, per kernel slot of the table (registry.h), the lowered name
struct RtcBlob {
  std::vector<std::pair<int, std::string>> names;
  std::vector<char> code;
};
const char kRtcMagic[] = "ASSET-HIP-RTC-1";   // (slot numbers are those of registry.h: a module is cached under a digest of csrc/*.h, asset_asrl_amd/jit.py)

bool rtc_write(const std::string& path, const RtcBlob& b) {
  const std::string tmp = path + ".tmp" + std::to_string(long(getpid()));
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return false;
  std::fprintf(f, "%s\n%zu\n", kRtcMagic, b.names.size());
  for (auto& n : b.names) std::fprintf(f, "%d %s\n", n.first, n.second.c_str());
  std::fprintf(f, "%zu\n", b.code.size());
  const bool ok = std::fwrite(b.code.data(), 1, b.code.size(), f) == b.code.size();
  std::fclose(f);
  if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) {   // (rename: a reader never sees half a file)
    std::remove(tmp.c_str());
    return false;
  }
  return true;
}
bool rtc_read(const std::string& path, RtcBlob& b) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  // lines of any length: the mangled name of a bundle kernel over eight user-named functors runs to kilobytes
  auto getline = [f](std::string& out) {
    out.clear();
    for (int c; (c = std::fgetc(f)) != EOF;) {
      if (c == '\n') return true;
      out.push_back(char(c));
    }
    return !out.empty();
  };
  std::string line;
  size_t n = 0, bytes = 0;
  bool ok = getline(line) && !std::strncmp(line.c_str(), kRtcMagic, sizeof kRtcMagic - 1) && getline(line) &&
            std::sscanf(line.c_str(), "%zu", &n) == 1;
  for (size_t i = 0; ok && i < n; i++) {
    int slot = -1, used = 0;
    ok = getline(line) && std::sscanf(line.c_str(), "%d %n", &slot, &used) == 1 && used > 0 && size_t(used) < line.size() &&
         slot >= 0 && slot < asset_hip::K_COUNT && line.find(' ', used) == std::string::npos;
    if (ok) b.names.emplace_back(slot, line.substr(used));
  }
  ok = ok && getline(line) && std::sscanf(line.c_str(), "%zu", &bytes) == 1 && bytes > 0;
  if (ok) {
    b.code.resize(bytes);
    ok = std::fread(b.code.data(), 1, bytes, f) == bytes;
  }
  std::fclose(f);
  return ok;
}

int rtc_compile(const char* source, const char* functor, int kind, int mode, int blocked, int seg_per_group,
                const char* const* options, int noptions, RtcBlob& out) {
  hiprtcProgram prog = nullptr;
  if (hiprtcCreateProgram(&prog, source, "asset_hip_plugin.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
    return fail(ASSET_HIP_ECOMPILE, "hiprtcCreateProgram failed");
  std::vector<std::pair<int, std::string>> exprs;
  for (int slot = 0; slot < asset_hip::K_COUNT; slot++) {
    const std::string ex = asset_hip::rtc_kernel_expr(slot, kind, functor, mode, blocked != 0, seg_per_group);
    if (ex.empty()) continue;
    exprs.emplace_back(slot, ex);
    if (hiprtcAddNameExpression(prog, ex.c_str()) != HIPRTC_SUCCESS) {
      hiprtcDestroyProgram(&prog);
      return fail(ASSET_HIP_ECOMPILE, "hiprtcAddNameExpression(" + ex + ") failed");
    }
  }
  const hiprtcResult rc = hiprtcCompileProgram(prog, noptions, const_cast<const char**>(options));
  if (rc != HIPRTC_SUCCESS) {
    size_t n = 0;
    std::string log;
    if (hiprtcGetProgramLogSize(prog, &n) == HIPRTC_SUCCESS && n > 1) {
      log.resize(n);
      hiprtcGetProgramLog(prog, &log[0]);
    }
    hiprtcDestroyProgram(&prog);
    if (log.size() > 6000) log = log.substr(0, 3000) + "\n...\n" + log.substr(log.size() - 3000);
    return fail(ASSET_HIP_ECOMPILE, std::string("hiprtc: ") + hiprtcGetErrorString(rc) + "\n" + log);
  }
  size_t bytes = 0;
  if (hiprtcGetCodeSize(prog, &bytes) != HIPRTC_SUCCESS || !bytes) {
    hiprtcDestroyProgram(&prog);
    return fail(ASSET_HIP_ECOMPILE, "hiprtcGetCodeSize failed");
  }
  out.code.resize(bytes);
  hiprtcGetCode(prog, out.code.data());
  for (auto& ex : exprs) {
    const char* low = nullptr;
    if (hiprtcGetLoweredName(prog, ex.second.c_str(), &low) != HIPRTC_SUCCESS || !low) {
      hiprtcDestroyProgram(&prog);
      return fail(ASSET_HIP_ECOMPILE, "hiprtcGetLoweredName(" + ex.second + ") failed");
    }
    out.names.emplace_back(ex.first, low);
  }
  hiprtcDestroyProgram(&prog);
  return 0;
}
}  // namespace

int asset_hip_jit_compile(const char* source, const char* functor, int kind, int mode, int blocked, int seg_per_group,
                          const char* const* options, int noptions, const char* cache_path) {
  if (!source || !functor || !cache_path || kind < 1 || kind > 3) return fail(ASSET_HIP_EINVAL, "bad jit arguments");
  RtcBlob blob;
  const int rc = rtc_compile(source, functor, kind, mode, blocked, seg_per_group, options, noptions, blob);
  if (rc) return rc;
  if (!rtc_write(cache_path, blob)) return fail(ASSET_HIP_EINVAL, std::string("cannot write ") + cache_path);
  return 0;
}

int asset_hip_jit_plugin(const char* name, const char* source, const char* functor, int kind, int mode, int blocked,
                         int seg_per_group, const char* const* options, int noptions, const char* cache_path) {
  if (!name || !functor || kind < 1 || kind > 3) return fail(ASSET_HIP_EINVAL, "bad jit arguments");
  if (find_entry(name, kind >= 2 ? ASSET_HIP_FUNCTION : mode, kind >= 2 ? 0 : blocked)) return 0;
  RtcBlob blob;
  if (!(cache_path && rtc_read(cache_path, blob))) {
    blob = RtcBlob();
    if (!source) return fail(ASSET_HIP_EINVAL, std::string("no compiled module at ") + (cache_path ? cache_path : "(null)") + " and no source");
    const int rc = rtc_compile(source, functor, kind, mode, blocked, seg_per_group, options, noptions, blob);
    if (rc) return rc;
    // (a cache that cannot be written -- a read-only install -- costs the next process a recompilation, nothing else)
    if (cache_path && !rtc_write(cache_path, blob)) std::fprintf(stderr, "asset_hip: cannot write the module cache %s\n", cache_path);
  }
  // The module stays with the process: its code object is loaded on every device a handle uses it on (registry.h:
  // RtcModule) -- here on the current one, to read its meta table.
  // (owned here until the entry is registered: every failure path below unloads the module and frees the code object)
  std::unique_ptr<asset_hip::RtcModule> rtc(new asset_hip::RtcModule());
  rtc->code.swap(blob.code);
  rtc->names.swap(blob.names);
  hipModule_t mod = nullptr;
  hipError_t e = rtc->module_on_current_device(&mod);
  if (e != hipSuccess) return hipfail(e, "loading the run-time module (hipModuleLoadData / hipModuleGetFunction)");
  std::unique_ptr<asset_hip::KernelTable> table(new asset_hip::KernelTable());
  hipDeviceptr_t dmeta = nullptr;
  size_t mbytes = 0;
  e = hipModuleGetGlobal(&dmeta, &mbytes, mod, "asset_rtc_meta");
  if (e != hipSuccess || mbytes != sizeof table->meta)
    return fail(ASSET_HIP_ECOMPILE, "the module has no asset_rtc_meta table of the expected size (rtc_device.h)");
  if ((e = hipMemcpy(table->meta, reinterpret_cast<void*>(dmeta), sizeof table->meta, hipMemcpyDeviceToHost)) != hipSuccess)
    return hipfail(e, "reading asset_rtc_meta");
  if (table->meta[asset_hip::MF_KIND] != kind || (kind == 1 && (table->meta[asset_hip::MF_MODE] != mode ||
                                                               table->meta[asset_hip::MF_BLOCKED] != (blocked ? 1 : 0))))
    return fail(ASSET_HIP_EINVAL, "the module was compiled for another transcription / kind than requested");
  for (auto& n : rtc->names) {
    table->k[n.first].rtc = rtc.get();
    table->k[n.first].slot = n.first;
  }
  rtc.release();                        // the module and its table stay with the process from here on
  auto* ke = new asset_hip::KernelEntry();
  asset_hip::entry_from_table(*ke, strdup(name), table.release());
  ke->next = asset_hip::registry_head();
  asset_hip::registry_head() = ke;
  return 0;
}

int asset_hip_load_plugin(const char* path) {
  if (!path) return fail(ASSET_HIP_EINVAL, "null plugin path");
  void* so = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!so) return fail(ASSET_HIP_EINVAL, std::string("dlopen failed: ") + dlerror());
  using entries_fn = asset_hip::KernelEntry* (*)();
  auto fn = reinterpret_cast<entries_fn>(dlsym(so, "asset_hip_plugin_entries"));
  if (!fn) {
    dlclose(so);
    return fail(ASSET_HIP_EINVAL, std::string(path) + " does not export asset_hip_plugin_entries");
  }
  int added = 0;
  for (asset_hip::KernelEntry* e = fn(); e;) {   // the plugin stays loaded: its entries and device code live in it
    asset_hip::KernelEntry* nx = e->next;
    if (!find_entry(e->ode, e->mode, e->blocked)) {
      e->next = asset_hip::registry_head();
      asset_hip::registry_head() = e;
      added++;
    }
    e = nx;
  }
  return added;
}

int asset_hip_has_kernel(const char* ode, int mode, int blocked) {
  return (ode && find_entry(ode, mode, blocked)) ? 1 : 0;
}

int asset_hip_lgl_table(int cs, const char* which, double* out, int cap) {
  if (cs < 2 || cs > 4 || !which || !out) return fail(ASSET_HIP_EINVAL, "bad lgl table query");
  const asset_hip::LglTab& t = asset_hip::h_lgl_tab[cs - 2];
  const int K = cs - 1;
  const double* src = nullptr;
  int rows = 1, cols = 0;
  if (!std::strcmp(which, "tc")) src = t.tc, cols = cs;
  else if (!std::strcmp(which, "s")) src = t.s, cols = K;
  else if (!std::strcmp(which, "E")) src = t.E, cols = K;
  else {
    rows = K, cols = cs;
    if (!std::strcmp(which, "A")) src = &t.A[0][0];
    else if (!std::strcmp(which, "B")) src = &t.B[0][0];
    else if (!std::strcmp(which, "U")) src = &t.U[0][0];
    else if (!std::strcmp(which, "C")) src = &t.C[0][0];
    else if (!std::strcmp(which, "D")) src = &t.D[0][0];
    else return fail(ASSET_HIP_EINVAL, "unknown table name");
  }
  if (cap < rows * cols) return fail(ASSET_HIP_EINVAL, "output buffer too small");
  for (int i = 0; i < rows; i++)
    for (int j = 0; j < cols; j++) out[i * cols + j] = (rows == 1) ? src[j] : src[i * 4 + j];
  return rows * cols;
}

// Index tables of a handle: bounds check (the kernels trust them), upload, run detection; buffers that depend on the number of
// applications are kept while they fit and re-allocated otherwise; everything derived from the OLD tables is dropped.
static int bind_tables(asset_hip_defect_t h, int nseg, const int32_t* vindex, const int32_t* cindex, int n_primal, int n_equal) {
  const asset_hip::KernelEntry* ke = h->ke;
  const size_t nv = size_t(ke->ir) * nseg, nc = size_t(ke->orr) * nseg;
  for (size_t i = 0; i < nv; i++)
    if (vindex[i] < 0 || vindex[i] >= n_primal) return fail(ASSET_HIP_ERANGE, "vindex entry out of range");
  for (size_t i = 0; i < nc; i++)
    if (cindex[i] < 0 || cindex[i] >= n_equal) return fail(ASSET_HIP_ERANGE, "cindex entry out of range");
  auto drop = [](auto*& p) { if (p) { (void)hipFree(p); p = nullptr; } };
  if (h->stream) HIP_TRY(hipStreamSynchronize(h->stream));       // (nothing of the old mesh is in flight on the handle's own stream ...
  if (h->last_stream_used) {                                     //  ... nor on the caller's stream of the last *_device call;
    if (hipStreamSynchronize(h->last_stream) != hipSuccess) (void)hipGetLastError();   //  a stream the caller has destroyed since is drained)
    h->last_stream_used = false;
  }
  // FAILURE-ATOMIC: every new buffer is allocated and filled through locals; the handle is touched only once all of that has succeeded.
  // A failed re-bind (out of device memory on a grown mesh) leaves the handle exactly as it was -- old mesh, old tables, still usable.
  int* nvi = nullptr;
  int* nci = nullptr;
  double* nwork = nullptr;
  int cap = h->cap_seg;
  const bool grow = nseg > h->cap_seg;
  auto undo = [&](hipError_t e, const char* what) {
    if (grow) { if (nvi) (void)hipFree(nvi); if (nci) (void)hipFree(nci); if (nwork) (void)hipFree(nwork); }
    return hipfail(e, what);
  };
  hipError_t e;
  if (grow) {                                                    // grow: index tables, workspace, block staging
    cap = h->cap_seg > 0 ? std::max(nseg, h->cap_seg + h->cap_seg / 4) : nseg;   // (re-meshing grows by steps)
    if ((e = hipMalloc(&nvi, size_t(ke->ir) * cap * sizeof(int))) != hipSuccess) return undo(e, "hipMalloc(vindex)");
    if ((e = hipMalloc(&nci, size_t(ke->orr) * cap * sizeof(int))) != hipSuccess) return undo(e, "hipMalloc(cindex)");
    if (ke->work_doubles) {
      if ((e = hipMalloc(&nwork, size_t(cap) * ke->work_doubles * sizeof(double))) != hipSuccess) return undo(e, "hipMalloc(workspace)");
      // sections no kernel writes must read as zero (the interior-point sections of a Trapezoidal slot, defect_dims.h)
      if ((e = hipMemset(nwork, 0, size_t(cap) * ke->work_doubles * sizeof(double))) != hipSuccess) return undo(e, "hipMemset(workspace)");
    }
  } else {
    nvi = h->d_vindex, nci = h->d_cindex;
  }
  // (when the mesh still fits the kept tables are overwritten in place: both streams were drained above, and a failed copy into them
  //  poisons the handle -- nseg = 0 -- instead of leaving half-written tables behind an old segment count)
  if ((e = hipMemcpy(nvi, vindex, nv * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) { if (!grow) h->nseg = 0; return undo(e, "hipMemcpy(vindex)"); }
  if ((e = hipMemcpy(nci, cindex, nc * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) { if (!grow) h->nseg = 0; return undo(e, "hipMemcpy(cindex)"); }
  if (grow) {
    drop(h->d_vindex), drop(h->d_cindex), drop(h->d_work), drop(h->d_fx), drop(h->d_agx), drop(h->d_kkt);
    h->d_vindex = nvi, h->d_cindex = nci, h->d_work = nwork, h->cap_seg = cap;
  }
  if (n_primal > h->cap_primal) drop(h->d_X), h->cap_primal = n_primal;
  if (n_equal > h->cap_equal) drop(h->d_L), h->cap_equal = n_equal;
  h->h_vindex.assign(vindex, vindex + nv);
  h->h_cindex.assign(cindex, cindex + nc);
  {   // rows that are runs with a constant stride between applications (EvalArgs::affine)
    const int ir = ke->ir, orr = ke->orr, ns = nseg;
    const int v0 = vindex[0], c0 = cindex[0];
    const int vs = ns > 1 ? vindex[ir] - v0 : 0, cs = ns > 1 ? cindex[orr] - c0 : 0;
    bool ok = true;
    for (int s = 0; s < ns && ok; s++) {
      for (int k = 0; k < ir && ok; k++) ok = vindex[size_t(s) * ir + k] == v0 + s * vs + k;
      for (int k = 0; k < orr && ok; k++) ok = cindex[size_t(s) * orr + k] == c0 + s * cs + k;
    }
    h->affine = ok ? 1 : 0, h->aff_v0 = v0, h->aff_vs = vs, h->aff_c0 = c0, h->aff_cs = cs;
  }
  // derived from the old tables: the KKT map and its staging, the RHS gather tables, per-application constants, block buffers
  drop(h->d_map), drop(h->d_values), drop(h->d_stage), drop(h->d_multi_ptr), drop(h->d_multi_loc), drop(h->d_aconst);
  drop(h->d_fx_rows), drop(h->d_fx_ptr), drop(h->d_fx_src), drop(h->d_gx_rows), drop(h->d_gx_ptr), drop(h->d_gx_src);
  drop(h->d_fxb), drop(h->d_agxb);
  if (h->h_values) { (void)hipHostFree(h->h_values); h->h_values = nullptr; }
  h->map_len = 0, h->value_lo = h->value_hi = h->nvalues = 0, h->nmulti = 0, h->nstage = 0;
  h->n_fx_rows = h->fx_long_from = h->n_gx_rows = h->gx_long_from = 0, h->rhs_tables_ready = false;
  h->nseg = nseg, h->n_primal = n_primal, h->n_equal = n_equal;
  return 0;
}

int asset_hip_defect_create(const asset_hip_defect_desc* d, asset_hip_defect_t* out) {
  if (!d || !out) return fail(ASSET_HIP_EINVAL, "null descriptor / output");
  *out = nullptr;
  if (!d->ode || !d->vindex || !d->cindex || d->nseg <= 0 || d->n_primal <= 0 || d->n_equal <= 0)
    return fail(ASSET_HIP_EINVAL, "descriptor fields missing or non-positive");
  const asset_hip::KernelEntry* ke = find_entry(d->ode, d->mode, d->blocked);
  if (!ke) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "no device code compiled for ode='%s' mode=%d blocked=%d", d->ode, d->mode,
                  d->blocked);
    return fail(ASSET_HIP_ENOODE, buf);
  }
  if (ke->table->meta[asset_hip::MF_KIND] == 3) return fail(ASSET_HIP_EINVAL, "a bundle is launched through asset_hip_bundle_*, it is not a function");
  {   // (before anything is allocated: the commonest set-up error)
    const size_t nv = size_t(ke->ir) * d->nseg, nc = size_t(ke->orr) * d->nseg;
    for (size_t i = 0; i < nv; i++)
      if (d->vindex[i] < 0 || d->vindex[i] >= d->n_primal) return fail(ASSET_HIP_ERANGE, "vindex entry out of range");
    for (size_t i = 0; i < nc; i++)
      if (d->cindex[i] < 0 || d->cindex[i] >= d->n_equal) return fail(ASSET_HIP_ERANGE, "cindex entry out of range");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ASSET_HIP_ENODEV, "no HIP device visible: the evaluator has no CPU fallback");
  if (d->device < 0 || d->device >= ndev) return fail(ASSET_HIP_EINVAL, "device ordinal out of range");
  HIP_TRY(hipSetDevice(d->device));
  asset_hip_defect* h = new (std::nothrow) asset_hip_defect;
  if (!h) return fail(ASSET_HIP_EINVAL, "out of host memory");
  h->ke = ke, h->device = d->device;
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, d->device);
  const int cus = (e == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  h->cus = cus;
  auto bail = [&](hipError_t err, const char* w) {
    int rc = hipfail(err, w);
    asset_hip_defect_destroy(h);
    return rc;
  };
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
  {
    const int rc = bind_tables(h, d->nseg, d->vindex, d->cindex, d->n_primal, d->n_equal);
    if (rc) {
      asset_hip_defect_destroy(h);
      return rc;
    }
  }
  // per-lane constants of the dense stage: computed here, once
    for (int level = 0; level <= 2; level++) {   // (0: the record of the resident kernel)
      const size_t nb = asset_hip::entry_lane_bytes(ke, level);
      if (!nb) continue;
      // ASSET_LANE_REPLICAS copies: every workgroup of the dense stage loads the whole table when it starts, all at the
      // same moment -- with one copy that is thousands of requests for the same few hundred cache lines, which the L2
      // channels holding them serve one after the other; workgroup b reads copy b % ASSET_LANE_REPLICAS.
      if ((e = hipMalloc(&h->d_lane[level], nb * ASSET_LANE_REPLICAS)) != hipSuccess) return bail(e, "hipMalloc(lane constants)");
      if ((e = asset_hip::entry_lane_setup(ke, level, h->d_lane[level], h->stream)) != hipSuccess) return bail(e, "lane_setup_kernel");
      for (int r = 1; r < ASSET_LANE_REPLICAS; r++)
        if ((e = hipMemcpyAsync(static_cast<char*>(h->d_lane[level]) + size_t(r) * nb, h->d_lane[level], nb,
                                hipMemcpyDeviceToDevice, h->stream)) != hipSuccess)
          return bail(e, "hipMemcpy(lane constants)");
    }
  if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return bail(e, "lane_setup_kernel");
  if ((e = hipEventCreate(&h->ev0)) != hipSuccess) return bail(e, "hipEventCreate");
  if ((e = hipEventCreate(&h->ev1)) != hipSuccess) return bail(e, "hipEventCreate");
  *out = h;
  return 0;
}

int asset_hip_defect_rebind(asset_hip_defect_t h, int nseg, const int32_t* vindex, const int32_t* cindex, int n_primal, int n_equal) {
  if (!h || !vindex || !cindex || nseg <= 0 || n_primal <= 0 || n_equal <= 0) return fail(ASSET_HIP_EINVAL, "bad rebind arguments");
  if (h->bundles > 0) return fail(ASSET_HIP_EINVAL, "the handle is a member of a bundle: destroy the bundle before re-binding");
  HIP_TRY(hipSetDevice(h->device));
  return bind_tables(h, nseg, vindex, cindex, n_primal, n_equal);
}

void asset_hip_defect_destroy(asset_hip_defect_t h) {
  if (!h) return;
  if (h->bundles > 0) {   // a bundle launches through this handle's tables and buffers: it lives until that bundle is gone
    h->destroy_pending = true;
    return;
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->d_vindex, (void*)h->d_cindex, (void*)h->d_X, (void*)h->d_L, (void*)h->d_fx,
                  (void*)h->d_agx, (void*)h->d_kkt, (void*)h->d_work, (void*)h->d_map, (void*)h->d_values, (void*)h->d_aconst,
                  (void*)h->d_stage, (void*)h->d_multi_ptr, (void*)h->d_multi_loc, (void*)h->d_fx_rows, (void*)h->d_fx_ptr,
                  (void*)h->d_fx_src, (void*)h->d_gx_rows, (void*)h->d_gx_ptr, (void*)h->d_gx_src, (void*)h->d_fxb, (void*)h->d_agxb,
                  h->d_lane[0], h->d_lane[1], h->d_lane[2]})
    if (p) (void)hipFree(p);
  if (h->h_values) (void)hipHostFree(h->h_values);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int asset_hip_defect_sizes(asset_hip_defect_t h, int* irows, int* orows, int* nkkt) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (irows) *irows = h->ke->ir;
  if (orows) *orows = h->ke->orr;
  if (nkkt) *nkkt = h->ke->nkkt;
  return 0;
}

// The order of a block's slots (defect_dims.h: Dims::KL, hcol / jcol -- the same arithmetic, on the host)
static int entry_kkt_layout(const asset_hip::KernelEntry* ke, int* stride, int32_t* rows, int32_t* cols) {
  const int IR = ke->ir, OR = ke->orr, KS = ke->kstride, kl = ke->kl;
  if (stride) *stride = KS;
  if (!rows && !cols) return kl;
  if (!rows || !cols) return fail(ASSET_HIP_EINVAL, "rows and cols go together");
  for (int k = 0; k < KS; k++) rows[k] = cols[k] = -1;
  const int hoff = kl ? (OR * IR + 15) / 16 * 16 : 0, hca = kl ? IR - 1 : IR + OR - 1;
  for (int c = 0; c < IR; c++) {
    const int hc = hoff + c * hca - c * (c - 1) / 2, jc = kl ? c * OR : hc + IR;
    for (int r = c; r < IR; r++) rows[hc + r] = r, cols[hc + r] = c;
    for (int j = 0; j < OR; j++) rows[jc + j] = IR + j, cols[jc + j] = c;
  }
  return kl;
}
int asset_hip_defect_kkt_layout(asset_hip_defect_t h, int* stride, int32_t* rows, int32_t* cols) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  return entry_kkt_layout(h->ke, stride, rows, cols);
}
int asset_hip_kkt_layout(const char* ode, int mode, int blocked, int* nkkt, int* stride, int32_t* rows, int32_t* cols) {
  const asset_hip::KernelEntry* ke = ode ? find_entry(ode, mode, blocked) : nullptr;
  if (!ke) return fail(ASSET_HIP_ENOODE, "no device code compiled for this (ode, mode, blocked)");
  if (nkkt) *nkkt = ke->nkkt;
  return entry_kkt_layout(ke, stride, rows, cols);
}

// The launch plan (registry.h: plan_lgl) of one evaluation kind, with the default dispatch -- what a handle of `nseg` segments on
// a device of `cus` compute units launches when no tuning knob is in effect
static int entry_launch_plan(const asset_hip::KernelEntry* ke, int what, int assembled, int nseg, int cus, bool res_record,
                             asset_hip_launch_plan* out) {
  const int level = level_of(what);
  if (!out || level < 0 || (what & ~0xff) || (assembled && what < ASSET_HIP_JAC)) return fail(ASSET_HIP_EINVAL, "bad launch plan query");
  if (ke->table->meta[asset_hip::MF_KIND] != 1) return fail(ASSET_HIP_EINVAL, "launch plans are those of the transcriptions of an ODE");
  const bool adj = what == ASSET_HIP_CON_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD_HESS;
  asset_hip::LaunchPlan p;
  if (asset_hip::plan_lgl(*ke->table, asset_hip::PlanRequest{level, what >= ASSET_HIP_JAC && !assembled, assembled != 0, adj, res_record},
                          nseg, cus, asset_hip::Tuning(), p) != hipSuccess)
    return fail(ASSET_HIP_EINVAL, "bad launch plan query (nseg and cus are positive)");
  *out = asset_hip_launch_plan();
  out->nsteps = p.nsteps, out->units_gp = p.units_gp;
  for (int i = 0; i < p.nsteps; i++) {
    const asset_hip::PlanStep& s = p.step[i];
    if (!ke->table->k[s.slot]) return fail(ASSET_HIP_ENOODE, std::string("the plan names a kernel this shape lacks: ") + asset_hip::kslot_name(s.slot));
    out->step[i] = asset_hip_plan_step{s.slot, int(s.grid_x), int(s.grid_y), int(s.block), (long long)s.lds_bytes, s.extra, s.gp};
  }
  return 0;
}
int asset_hip_launch_plan_query(const char* ode, int mode, int blocked, int what, int assembled, int nseg, int cus,
                                asset_hip_launch_plan* out) {
  const asset_hip::KernelEntry* ke = ode ? find_entry(ode, mode, blocked) : nullptr;
  if (!ke) return fail(ASSET_HIP_ENOODE, "no device code compiled for this (ode, mode, blocked)");
  return entry_launch_plan(ke, what, assembled, nseg, cus, asset_hip::entry_lane_bytes(ke, 0) > 0, out);
}
int asset_hip_defect_launch_plan(asset_hip_defect_t h, int what, int assembled, asset_hip_launch_plan* out) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  return entry_launch_plan(h->ke, what, assembled, h->nseg, h->cus, h->d_lane[0] != nullptr, out);
}
const char* asset_hip_kernel_slot_name(int slot) { return asset_hip::kslot_name(slot); }
int asset_hip_kernel_slot_kinds(int slot) {
  int kinds = 0;
  for (int kind = 1; kind <= 3; kind++)
    if (!asset_hip::rtc_kernel_expr(slot, kind, "F", ASSET_HIP_LGL3, false, 1).empty()) kinds |= 1 << (kind - 1);
  return kinds;
}

// the kernel arguments of one evaluation of a handle (block kinds)
static int fill_args(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx, double* dagx,
                     double* dkkt, asset_hip::EvalArgs& a) {
  const int level = level_of(what);
  if (level < 0) return fail(ASSET_HIP_EINVAL, "unknown evaluation kind");
  if (h->nseg <= 0) return fail(ASSET_HIP_EINVAL, "the handle holds no mesh (a failed asset_hip_defect_rebind): re-bind it first");
  const int opts = what & ~0xff;
  what &= 0xff;
  if ((opts & ~ASSET_HIP_KEEP_HESSIAN_SLOTS) || (opts && what != ASSET_HIP_JAC && what != ASSET_HIP_JAC_ADJGRAD))
    return fail(ASSET_HIP_EINVAL, "ASSET_HIP_KEEP_HESSIAN_SLOTS goes with ASSET_HIP_JAC / ASSET_HIP_JAC_ADJGRAD only");
  // (honoured while the phase's blocks stay in the Infinity Cache; see include/asset_hip.h)
  // (wide shapes -- IR >= 64 -- skip whole lines: it pays at every size there)
  const bool keep_pays = h->ke->ir >= 64 || size_t(h->nseg) * size_t(h->ke->kstride) * sizeof(double) <= (size_t(192) << 20);
  a.flags = ((opts & ASSET_HIP_KEEP_HESSIAN_SLOTS) && keep_pays) ? 1 : 0;
  if (!dX) return fail(ASSET_HIP_EINVAL, "X is null");
  const bool needs_l = (what == ASSET_HIP_CON_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD_HESS);
  if (needs_l && !dL) return fail(ASSET_HIP_EINVAL, "L is null for an evaluation kind that contracts with multipliers");
  a.nseg = h->nseg;
  a.X = dX;
  a.L = needs_l ? dL : nullptr;
  a.vindex = h->d_vindex;
  a.cindex = h->d_cindex;
  a.FX = dfx;
  a.AGX = (what == ASSET_HIP_CON || what == ASSET_HIP_JAC) ? nullptr : dagx;
  a.KKT = (what >= ASSET_HIP_JAC) ? dkkt : nullptr;
  a.work = h->d_work;
  a.lane_consts = level >= 1 ? h->d_lane[level] : nullptr;
  a.lane_consts_res = h->d_lane[0];
  a.affine = asset_hip::tuning().no_affine ? 0 : h->affine, a.aff_v0 = h->aff_v0, a.aff_vs = h->aff_vs, a.aff_c0 = h->aff_c0, a.aff_cs = h->aff_cs;
  a.appl_consts = h->d_aconst;
  if (h->ke->naconst > 0 && !h->d_aconst)
    return fail(ASSET_HIP_EINVAL, "this function reads constants of its applications: call asset_hip_defect_set_appl_consts first");
  return 0;
}

static int launch(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx, double* dagx,
                  double* dkkt, hipStream_t st, double* d_values = nullptr) {
  if (st != h->stream) h->last_stream = st, h->last_stream_used = true;
  asset_hip::EvalArgs a;
  const int rc = fill_args(h, what, dX, dL, dfx, dagx, dkkt, a);
  if (rc) return rc;
  const int level = level_of(what);
  if (d_values) {                                                          // on-device assembly
    a.kmap = h->d_map, a.values = d_values, a.KKT = nullptr;
    a.stage = h->d_stage, a.nvalues = int(h->nvalues);
  }
  hipError_t e = asset_hip::entry_launch(h->ke, level, a, h->cus, st);
  if (e != hipSuccess) return hipfail(e, "kernel launch");
  if (d_values && h->nmulti > 0 && level >= 2) {   // the staged locations (Hessian entries only): fixed-order sums
    hipLaunchKernelGGL(asset_hip::asm_reduce_kernel, dim3(h->nmulti), dim3(256), 0, st, d_values, h->d_stage, h->d_multi_ptr,
                       h->d_multi_loc);
    if ((e = hipGetLastError()) != hipSuccess) return hipfail(e, "asm_reduce_kernel");
  }
  return 0;
}

int asset_hip_defect_eval_device(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx,
                                 double* dagx, double* dkkt, void* stream) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  return launch(h, what, dX, dL, dfx, dagx, dkkt, stream ? static_cast<hipStream_t>(stream) : h->stream);
}

// ---- bundles: several plain functions in one launch (func_kernels.h: func_bundle_kernel) ---------------------------------
struct asset_hip_bundle {
  const asset_hip::KernelEntry* ke = nullptr;
  std::vector<asset_hip_defect_t> members;
  int device = 0;
};

int asset_hip_bundle_create(const char* name, const asset_hip_defect_t* members, int n, asset_hip_bundle_t* out) {
  if (!name || !members || !out || n < 1 || n > asset_hip::BUNDLE_MAX) return fail(ASSET_HIP_EINVAL, "bad bundle arguments");
  const asset_hip::KernelEntry* ke = find_entry(name, ASSET_HIP_FUNCTION, 0);
  if (!ke || ke->table->meta[asset_hip::MF_KIND] != 3) return fail(ASSET_HIP_ENOODE, std::string("no compiled bundle '") + name + "'");
  if (ke->table->meta[asset_hip::MF_XV] != n) return fail(ASSET_HIP_EINVAL, "the bundle was compiled for another number of functions");
  for (int k = 0; k < n; k++) {
    const asset_hip_defect_t h = members[k];
    if (!h || h->ke->mode != ASSET_HIP_FUNCTION || h->ke->table->meta[asset_hip::MF_KIND] != 2)
      return fail(ASSET_HIP_EINVAL, "bundle members are handles of plain functions");
    if (h->device != members[0]->device) return fail(ASSET_HIP_EINVAL, "bundle members live on different devices");
    if (ke->table->meta[asset_hip::MF_BYTES_ODE + k] != (long long)(h->ke->ir) * 65536 + h->ke->orr)
      return fail(ASSET_HIP_EINVAL, "member " + std::to_string(k) + " does not have the sizes of the bundle's function " + std::to_string(k));
  }
  auto* b = new (std::nothrow) asset_hip_bundle();
  if (!b) return fail(ASSET_HIP_EINVAL, "out of memory");
  b->ke = ke, b->members.assign(members, members + n), b->device = members[0]->device;
  for (asset_hip_defect_t h : b->members) h->bundles++;
  *out = b;
  return 0;
}

void asset_hip_bundle_destroy(asset_hip_bundle_t b) {
  if (!b) return;
  for (asset_hip_defect_t h : b->members)
    if (--h->bundles == 0 && h->destroy_pending) asset_hip_defect_destroy(h);   // (its owner let go of it earlier)
  delete b;
}

int asset_hip_bundle_eval_device(asset_hip_bundle_t b, int what, const double* dX, const double* const* dL,
                                 double* const* d_fx, double* const* d_agx, double* const* d_kkt, void* stream) {
  if (!b || !d_fx) return fail(ASSET_HIP_EINVAL, "bad bundle arguments");
  const int level = level_of(what);
  if (level < 0) return fail(ASSET_HIP_EINVAL, "unknown evaluation kind");
  HIP_TRY(hipSetDevice(b->device));
  asset_hip::BundleArgs args;
  const int n = int(b->members.size());
  args.n = n;
  size_t shmem = 0;
  int blocks = 0;
  for (int k = 0; k < n; k++) {
    asset_hip_defect_t h = b->members[k];
    const int rc = fill_args(h, what, dX, dL ? dL[k] : nullptr, d_fx[k], d_agx ? d_agx[k] : nullptr, d_kkt ? d_kkt[k] : nullptr,
                             args.a[k]);
    if (rc) return rc;
    const long long* m = h->ke->table->meta;
    const bool staged = level >= 1 && m[asset_hip::MF_G] > 0;     // (as launch_func_table: the block kinds stage in LDS)
    const int apw = staged ? int(m[asset_hip::MF_G]) : 64;
    if (staged && size_t(m[asset_hip::MF_LDS_BYTES]) > shmem) shmem = size_t(m[asset_hip::MF_LDS_BYTES]);
    args.start[k] = blocks;
    blocks += (h->nseg + apw - 1) / apw;
  }
  for (int k = n; k <= asset_hip::BUNDLE_MAX; k++) args.start[k] = blocks;
  void* kargs[] = {&args};
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : b->members[0]->stream;
  const int slot = level == 0 ? asset_hip::K_BUNDLE0 : (level == 1 ? asset_hip::K_BUNDLE1 : asset_hip::K_BUNDLE2);
  hipError_t e = asset_hip::klaunch(b->ke->table->k[slot], dim3(blocks), dim3(64), shmem, st, kargs);
  if (e != hipSuccess) return hipfail(e, "bundle launch");
  return 0;
}

int asset_hip_defect_time_device(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx,
                                 double* dagx, double* dkkt, int warmup, int iters, float* ms_per_launch) {
  if (!h || !ms_per_launch || iters <= 0) return fail(ASSET_HIP_EINVAL, "bad timing arguments");
  HIP_TRY(hipSetDevice(h->device));
  for (int i = 0; i < warmup; i++) {
    int rc = launch(h, what, dX, dL, dfx, dagx, dkkt, h->stream);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  for (int i = 0; i < iters; i++) {
    int rc = launch(h, what, dX, dL, dfx, dagx, dkkt, h->stream);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  HIP_TRY(hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *ms_per_launch = ms / float(iters);
  return 0;
}

int asset_hip_defect_eval(asset_hip_defect_t h, int what, const double* X, const double* L, double* fx, double* agx,
                          double* kkt) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (!X) return fail(ASSET_HIP_EINVAL, "X is null");
  HIP_TRY(hipSetDevice(h->device));
  const size_t nfx = size_t(h->nseg) * h->ke->orr, nagx = size_t(h->nseg) * h->ke->ir,
               nkkt = size_t(h->nseg) * h->ke->kstride;   // (blocks in the handle's layout: asset_hip_defect_kkt_layout)
  if (!h->d_X) HIP_TRY(hipMalloc(&h->d_X, sizeof(double) * h->cap_primal));
  if (!h->d_L) HIP_TRY(hipMalloc(&h->d_L, sizeof(double) * h->cap_equal));
  if (fx && !h->d_fx) HIP_TRY(hipMalloc(&h->d_fx, sizeof(double) * size_t(h->cap_seg) * h->ke->orr));   // (sized for the handle's capacity: asset_hip_defect_rebind)
  if (agx && !h->d_agx) HIP_TRY(hipMalloc(&h->d_agx, sizeof(double) * size_t(h->cap_seg) * h->ke->ir));
  if (kkt && !h->d_kkt) HIP_TRY(hipMalloc(&h->d_kkt, sizeof(double) * size_t(h->cap_seg) * h->ke->kstride));
  HIP_TRY(hipMemcpyAsync(h->d_X, X, sizeof(double) * h->n_primal, hipMemcpyHostToDevice, h->stream));
  if (L) HIP_TRY(hipMemcpyAsync(h->d_L, L, sizeof(double) * h->n_equal, hipMemcpyHostToDevice, h->stream));
  int rc = launch(h, what, h->d_X, L ? h->d_L : nullptr, fx ? h->d_fx : nullptr, agx ? h->d_agx : nullptr,
                  kkt ? h->d_kkt : nullptr, h->stream);
  if (rc) return rc;
  const int level = level_of(what);
  what &= 0xff;
  if (fx) HIP_TRY(hipMemcpyAsync(fx, h->d_fx, sizeof(double) * nfx, hipMemcpyDeviceToHost, h->stream));
  if (agx && what != ASSET_HIP_CON && what != ASSET_HIP_JAC)
    HIP_TRY(hipMemcpyAsync(agx, h->d_agx, sizeof(double) * nagx, hipMemcpyDeviceToHost, h->stream));
  if (kkt && level >= 1 && what >= ASSET_HIP_JAC)
    HIP_TRY(hipMemcpyAsync(kkt, h->d_kkt, sizeof(double) * nkkt, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int asset_hip_defect_set_appl_consts(asset_hip_defect_t h, const double* consts, int per_application) {
  if (!h || !consts) return fail(ASSET_HIP_EINVAL, "null handle / constants");
  if (per_application != h->ke->naconst || per_application <= 0)
    return fail(ASSET_HIP_EINVAL, "the number of constants per application does not match the function");
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = size_t(h->nseg) * per_application;
  if (!h->d_aconst) HIP_TRY(hipMalloc(&h->d_aconst, n * sizeof(double)));
  HIP_TRY(hipMemcpy(h->d_aconst, consts, n * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int asset_hip_host_register(void* ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(ASSET_HIP_EINVAL, "null range");
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return 0;
}
int asset_hip_host_unregister(void* ptr) {
  if (!ptr) return fail(ASSET_HIP_EINVAL, "null range");
  HIP_TRY(hipHostUnregister(ptr));
  return 0;
}

// ---------------------------------------------------------------------------------------------- mesh error estimate

int asset_hip_mesh_error_deboor(const char* ode, int mode, int blocked, const double* traj, int nnodes, double* tsnd,
                                double* mesh_errors, double* mesh_dist, double* error_max, double* dist_max,
                                int device) {
  if (!ode || !traj || !tsnd || !mesh_errors || !mesh_dist) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = find_entry(ode, mode, blocked);
  if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no device code compiled for ode='") + ode + "' in this mode");
  if (!asset_hip::entry_has_mesh(ke)) return fail(ASSET_HIP_EINVAL, "this entry is not a transcription of an ODE");
  const int cs = asset_hip::mesh_scheme(mode).cs, n = ke->xv, N = ke->xv + 1 + ke->uv + ke->pv;
  const int nb = (nnodes - 1) / (cs - 1);
  if (nb < 2 || nb * (cs - 1) + 1 != nnodes)
    return fail(ASSET_HIP_EINVAL, "the trajectory must hold nb*(cs-1)+1 nodes with nb >= 2 blocks");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ASSET_HIP_ENODEV, "no HIP device visible: the estimator has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(ASSET_HIP_EINVAL, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  // one allocation: traj | yvec | hs | tsnd | errors | dist | error_max | dist_max
  const size_t sz_traj = size_t(nnodes) * N, sz_y = size_t(nb) * n, sz_e = size_t(nb + 1) * n;
  const size_t total = sz_traj + sz_y + nb + (nb + 1) + 2 * sz_e + 2 * size_t(nb + 1);
  double* buf = nullptr;
  HIP_TRY(hipMalloc(&buf, total * sizeof(double)));
  asset_hip::MeshArgs a;
  a.nb = nb;
  double* p = buf;
  a.traj = p, p += sz_traj;
  a.yvec = p, p += sz_y;
  a.hs = p, p += nb;
  a.tsnd = p, p += nb + 1;
  a.errors = p, p += sz_e;
  a.dist = p, p += sz_e;
  a.error_max = p, p += nb + 1;
  a.dist_max = p;
  auto done = [&](int rc) { (void)hipFree(buf); return rc; };
  hipError_t e = hipMemcpy(buf, traj, sz_traj * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) return done(hipfail(e, "hipMemcpy(traj)"));
  if ((e = asset_hip::entry_mesh(ke, a, nullptr)) != hipSuccess) return done(hipfail(e, "mesh kernels"));
  if ((e = hipMemcpy(tsnd, a.tsnd, (nb + 1) * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(mesh_errors, a.errors, sz_e * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess ||
      (e = hipMemcpy(mesh_dist, a.dist, sz_e * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
    return done(hipfail(e, "hipMemcpy(results)"));
  if (error_max && (e = hipMemcpy(error_max, a.error_max, (nb + 1) * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
    return done(hipfail(e, "hipMemcpy(error_max)"));
  if (dist_max && (e = hipMemcpy(dist_max, a.dist_max, (nb + 1) * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess)
    return done(hipfail(e, "hipMemcpy(dist_max)"));
  return done(0);
}

// ---------------------------------------------------------------------------------------------- trajectory table

struct asset_hip_traj_table {
  const asset_hip::KernelEntry* ke = nullptr;
  int nb = 0, nnodes = 0, N = 0, n = 0, device = 0, cus = 256;
  double t0 = 0.0, tf = 0.0;
  double* d_buf = nullptr;     // traj | xdot | tb, resident
  asset_hip::InterpArgs a{};
  // staging of the host-pointer entry point (grown on demand): times | out | dout, and the counter
  double* d_stage = nullptr;
  long long cap_q = 0;
  unsigned long long* d_count = nullptr;
  hipStream_t stream = nullptr;
};

int asset_hip_traj_table_create(const char* ode, int mode, int blocked, const double* traj, int nnodes, int device,
                                asset_hip_traj_table_t* out) {
  if (!ode || !traj || !out) return fail(ASSET_HIP_EINVAL, "null argument");
  *out = nullptr;
  const asset_hip::KernelEntry* ke = find_entry(ode, mode, blocked);
  if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no device code compiled for ode='") + ode + "' in this mode");
  if (ke->table->meta[asset_hip::MF_KIND] != 1 || !asset_hip::entry_has_interp(ke))
    return fail(ASSET_HIP_EINVAL, "this entry has no trajectory-table kernels (it is not a transcription of an ODE)");
  const int K = asset_hip::interp_basis(mode).cs - 1, n = ke->xv, N = ke->xv + 1 + ke->uv + ke->pv;
  if (nnodes < 2 || (nnodes - 1) % K != 0)
    return fail(ASSET_HIP_EINVAL, "the trajectory must hold nb*(cs-1)+1 nodes with nb >= 1 blocks");
  const int nb = (nnodes - 1) / K;
  for (size_t i = 0, e = size_t(nnodes) * N; i < e; i++)
    if (!std::isfinite(traj[i])) return fail(ASSET_HIP_EINVAL, "NaN or Inf in the trajectory");
  // the reference's two checkInput errors (LGLInterpTable.h:147-165)
  const double dirn = traj[size_t(nnodes - 1) * N + n] - traj[n];
  for (int j = 0; j + 1 < nnodes; j++) {
    const double d = traj[size_t(j + 1) * N + n] - traj[size_t(j) * N + n];
    if (d == 0.0) return fail(ASSET_HIP_EINVAL, "the trajectory holds duplicate times (node " + std::to_string(j) + ")");
    if ((d > 0.0) != (dirn > 0.0)) return fail(ASSET_HIP_EINVAL, "the trajectory's times are not monotonic (node " + std::to_string(j) + ")");
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ASSET_HIP_ENODEV, "no HIP device visible: the trajectory table has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(ASSET_HIP_EINVAL, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<asset_hip_traj_table> t(new (std::nothrow) asset_hip_traj_table());
  if (!t) return fail(ASSET_HIP_EINVAL, "out of host memory");
  t->ke = ke, t->nb = nb, t->nnodes = nnodes, t->N = N, t->n = n, t->device = device;
  t->t0 = traj[n], t->tf = traj[size_t(nnodes - 1) * N + n];
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) t->cus = prop.multiProcessorCount;
  const size_t sz_traj = size_t(nnodes) * N, sz_xd = size_t(nnodes) * n, total = sz_traj + sz_xd + size_t(nb) + 1;
  auto bail = [&](int rc) {
    if (t->d_buf) (void)hipFree(t->d_buf);
    if (t->d_count) (void)hipFree(t->d_count);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    return rc;
  };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking)) != hipSuccess) return bail(hipfail(e, "hipStreamCreate"));
  if ((e = hipMalloc(&t->d_buf, total * sizeof(double))) != hipSuccess) return bail(hipfail(e, "hipMalloc(table)"));
  if ((e = hipMalloc(&t->d_count, sizeof(unsigned long long))) != hipSuccess) return bail(hipfail(e, "hipMalloc(counter)"));
  t->a.nb = nb, t->a.nq = 0;
  t->a.traj = t->d_buf, t->a.xdot = t->d_buf + sz_traj, t->a.tb = t->d_buf + sz_traj + sz_xd;
  if ((e = hipMemcpyAsync(t->d_buf, traj, sz_traj * sizeof(double), hipMemcpyHostToDevice, t->stream)) != hipSuccess)
    return bail(hipfail(e, "hipMemcpy(traj)"));
  if ((e = asset_hip::entry_interp_table(ke, t->a, t->stream)) != hipSuccess) return bail(hipfail(e, "interp_xdot_kernel"));
  if ((e = hipStreamSynchronize(t->stream)) != hipSuccess) return bail(hipfail(e, "trajectory table set-up"));
  *out = t.release();
  return 0;
}

static int traj_table_launch(asset_hip_traj_table_t t, const double* d_times, long long n, int deriv, double* d_out,
                             double* d_dout, unsigned long long* d_count, hipStream_t st) {
  asset_hip::InterpArgs a = t->a;
  a.nq = n, a.times = d_times, a.out = d_out, a.dout = deriv ? d_dout : nullptr, a.n_outside = d_count;
  const hipError_t e = asset_hip::entry_interp(t->ke, a, t->cus, st);
  if (e != hipSuccess) return hipfail(e, "interp_eval_kernel");
  return 0;
}

int asset_hip_traj_table_interp_device(asset_hip_traj_table_t t, const double* d_times, long long n, int deriv, double* d_out,
                                       double* d_dout, unsigned long long* d_n_outside, void* stream) {
  if (!t) return fail(ASSET_HIP_EINVAL, "null table");
  if (n < 0 || (n > 0 && (!d_times || !d_out)) || (deriv && n > 0 && !d_dout)) return fail(ASSET_HIP_EINVAL, "bad interpolation arguments");
  HIP_TRY(hipSetDevice(t->device));
  return traj_table_launch(t, d_times, n, deriv, d_out, d_dout, d_n_outside, stream ? static_cast<hipStream_t>(stream) : t->stream);
}

int asset_hip_traj_table_interp(asset_hip_traj_table_t t, const double* times, long long n, int deriv, double* out, double* dout,
                                long long* n_outside) {
  if (!t) return fail(ASSET_HIP_EINVAL, "null table");
  if (n < 0 || (n > 0 && (!times || !out)) || (deriv && n > 0 && !dout)) return fail(ASSET_HIP_EINVAL, "bad interpolation arguments");
  if (n_outside) *n_outside = 0;
  if (n == 0) return 0;
  for (long long i = 0; i < n; i++)
    if (!std::isfinite(times[i])) return fail(ASSET_HIP_EINVAL, "NaN or Inf among the query times");
  HIP_TRY(hipSetDevice(t->device));
  const size_t N = size_t(t->N);
  if (n > t->cap_q) {   // times | out | dout
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (t->d_stage) (void)hipFree(t->d_stage);
    t->d_stage = nullptr, t->cap_q = 0;
    HIP_TRY(hipMalloc(&t->d_stage, size_t(n) * (1 + 2 * N) * sizeof(double)));
    t->cap_q = n;
  }
  double *d_times = t->d_stage, *d_out = d_times + t->cap_q, *d_dout = d_out + size_t(t->cap_q) * N;
  HIP_TRY(hipMemcpyAsync(d_times, times, size_t(n) * sizeof(double), hipMemcpyHostToDevice, t->stream));
  HIP_TRY(hipMemsetAsync(t->d_count, 0, sizeof(unsigned long long), t->stream));
  const int rc = traj_table_launch(t, d_times, n, deriv, d_out, d_dout, t->d_count, t->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, size_t(n) * N * sizeof(double), hipMemcpyDeviceToHost, t->stream));
  if (deriv) HIP_TRY(hipMemcpyAsync(dout, d_dout, size_t(n) * N * sizeof(double), hipMemcpyDeviceToHost, t->stream));
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, t->d_count, sizeof cnt, hipMemcpyDeviceToHost, t->stream));
  HIP_TRY(hipStreamSynchronize(t->stream));
  if (n_outside) *n_outside = (long long)cnt;
  return 0;
}

int asset_hip_traj_table_info(asset_hip_traj_table_t t, int* nblocks, int* ncols, double* t0, double* tf) {
  if (!t) return fail(ASSET_HIP_EINVAL, "null table");
  if (nblocks) *nblocks = t->nb;
  if (ncols) *ncols = t->N;
  if (t0) *t0 = t->t0;
  if (tf) *tf = t->tf;
  return 0;
}

void asset_hip_traj_table_destroy(asset_hip_traj_table_t t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  (void)hipDeviceSynchronize();          // (queries enqueued on the caller's streams still read the table)
  if (t->d_buf) (void)hipFree(t->d_buf);
  if (t->d_stage) (void)hipFree(t->d_stage);
  if (t->d_count) (void)hipFree(t->d_count);
  if (t->stream) (void)hipStreamDestroy(t->stream);
  delete t;
}

// ---------------------------------------------------------------------------------------------- on-device assembly

int asset_hip_defect_set_kkt_map(asset_hip_defect_t h, const int32_t* slot_locations, long long nvalues, int accumulate) {
  if (!h || !slot_locations || nvalues <= 0) return fail(ASSET_HIP_EINVAL, "bad kkt map arguments");
  HIP_TRY(hipSetDevice(h->device));
  const size_t nslots = size_t(h->nseg) * h->ke->nkkt;
  long long lo = nvalues, hi = 0;
  for (size_t i = 0; i < nslots; i++) {
    const long long m = slot_locations[i];
    if (m == -1) continue;   // a slot the caller does not want (the Jacobian slots of an objective: Hessian only)
    if (m < 0 || m >= nvalues) return fail(ASSET_HIP_ERANGE, "kkt slot location outside [0, nvalues) and not -1");
    lo = m < lo ? m : lo;
    hi = m + 1 > hi ? m + 1 : hi;
  }
  if (hi <= lo) return fail(ASSET_HIP_EINVAL, "kkt map keeps no slot");
  // a location used by exactly one slot is stored to; one that two slots share is added to atomically (two terms: the
  // order cannot matter); one that three or more share is STAGED -- every such slot gets a cell of its own and the cells
  // of a location are summed in slot order afterwards (encoding: defect_dims.h, EvalArgs::kmap / stage).  In accumulate
  // mode every slot adds atomically into whatever the array holds.
  std::vector<unsigned char> uses(accumulate ? 0 : size_t(hi - lo), 0);
  if (!accumulate)
    for (size_t i = 0; i < nslots; i++) {
      if (slot_locations[i] < 0) continue;
      unsigned char& u = uses[size_t(slot_locations[i] - lo)];
      if (u < 3) u++;
    }
  // only Hessian slots are staged (a Jacobian slot's location belongs to one constraint row of one application; and the
  // Jacobian-only evaluation kinds write no Hessian entry, so they must not leave cells half-filled)
  const int IRk = h->ke->ir, ORk = h->ke->orr, NKk = h->ke->nkkt;
  std::vector<unsigned char> is_h(NKk, 0);
  for (int c = 0, k = 0; c < IRk; c++) {
    for (int j = c; j < IRk; j++) is_h[k++] = 1;
    k += ORk;
  }
  auto staged = [&](size_t i) {
    const int32_t m = slot_locations[i];
    return m >= 0 && is_h[i % size_t(NKk)] && uses[size_t(m - lo)] >= 3;
  };
  std::vector<int32_t> multi_loc, multi_ptr(1, 0);
  std::unordered_map<int32_t, int> multi_of;           // location -> index in multi_loc
  if (!accumulate) {
    for (size_t i = 0; i < nslots; i++) {
      const int32_t m = slot_locations[i];
      if (staged(i) && multi_of.emplace(m, 0).second) multi_loc.push_back(m);
    }
    std::sort(multi_loc.begin(), multi_loc.end());
    for (size_t l = 0; l < multi_loc.size(); l++) multi_of[multi_loc[l]] = int(l);
    std::vector<int> cnt(multi_loc.size(), 0);
    for (size_t i = 0; i < nslots; i++) {
      if (staged(i)) cnt[multi_of[slot_locations[i]]]++;
    }
    multi_ptr.resize(multi_loc.size() + 1);
    for (size_t l = 0; l < multi_loc.size(); l++) multi_ptr[l + 1] = multi_ptr[l] + cnt[l];
    if (nvalues + (long long)multi_ptr.back() + 2 > 2147483647LL)
      return fail(ASSET_HIP_ERANGE, "value array + staging cells exceed the 32-bit map range");
  }
  std::vector<int32_t> enc(nslots);                     // map word of every slot, slot order (cells are handed out in it)
  {
    std::vector<int> fill(multi_ptr.begin(), multi_ptr.end() - (multi_ptr.size() > 1 ? 1 : 0));
    for (size_t i = 0; i < nslots; i++) {
      const int32_t m = slot_locations[i];
      if (m < 0) enc[i] = -1;
      else if (accumulate) enc[i] = -(m + 2);
      else {
        const unsigned char u = uses[size_t(m - lo)];
        if (u == 1) enc[i] = m;
        else if (!staged(i) || !multi_of.count(m)) enc[i] = -(m + 2);   // (a location staged for its Hessian slots takes no other)
        else enc[i] = -(int32_t(nvalues) + fill[multi_of[m]]++ + 2);
      }
    }
  }
  std::vector<int32_t> map;
  if (h->ke->mode == ASSET_HIP_FUNCTION) {   // plain functions place their entries slot by slot (func_kernels.h)
    map = enc;
  } else {
    // fragment order of the LGL dense stage (defect_kernels.h, ASM): for every segment (4*tiles) rows of 64 lanes;
    // lane (lr = l & 15, lk = l >> 4), entry v of an accumulator tile is block column c = 16ct + lk + 4v and row
    // r = 16rt + lr (H, lower-triangle tiles first, tix = rt(rt+1)/2 + ct) or defect row jr = 16jt + lr
    // (J, tile ct*TJ + jt); -1 where that entry is no KKT slot.
    const int IR = h->ke->ir, OR = h->ke->orr, NK = h->ke->nkkt;
    const int TI = (IR + 15) / 16, TJ = (OR + 15) / 16, NTH = TI * (TI + 1) / 2, NF = (NTH + TI * TJ) * 4;
    std::vector<int32_t> slot_of(size_t(NF) * 64, -1);
    for (int l = 0; l < 64; l++) {
      const int lr = l & 15, lk = l >> 4;
      for (int ct = 0; ct < TI; ct++)
        for (int v = 0; v < 4; v++) {
          const int c = 16 * ct + lk + 4 * v;
          if (c >= IR) continue;
          const int cst = c * (IR + OR) - c * (c - 1) / 2;   // first slot of block column c
          for (int rt = ct; rt < TI; rt++) {
            const int r = 16 * rt + lr;
            if (r < IR && r >= c) slot_of[size_t((rt * (rt + 1) / 2 + ct) * 4 + v) * 64 + l] = cst + (r - c);
          }
          for (int jt = 0; jt < TJ; jt++) {
            const int jr = 16 * jt + lr;
            if (jr < OR) slot_of[size_t((NTH + ct * TJ + jt) * 4 + v) * 64 + l] = cst + (IR - c) + jr;
          }
        }
    }
    map.resize(size_t(h->nseg) * NF * 64);
    for (int V = 0; V < h->nseg; V++) {
      const int32_t* loc = slot_locations + size_t(V) * NK;
      int32_t* dst = map.data() + size_t(V) * NF * 64;
      const int32_t* encV = enc.data() + size_t(V) * NK;
      (void)loc;
      for (size_t e = 0; e < size_t(NF) * 64; e++) dst[e] = slot_of[e] < 0 ? -1 : encV[slot_of[e]];
    }
  }
  if (h->d_map && h->map_len != map.size()) {
    (void)hipFree(h->d_map);
    h->d_map = nullptr;
  }
  if (!h->d_map) HIP_TRY(hipMalloc(&h->d_map, map.size() * sizeof(int32_t)));
  h->map_len = map.size();
  HIP_TRY(hipMemcpy(h->d_map, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (h->d_values && (hi - lo) != (h->value_hi - h->value_lo)) {
    (void)hipFree(h->d_values);
    (void)hipHostFree(h->h_values);
    h->d_values = nullptr, h->h_values = nullptr;
  }
  h->value_lo = lo, h->value_hi = hi, h->nvalues = nvalues;
  // staging cells and the reduction lists
  for (void* p : {(void*)h->d_stage, (void*)h->d_multi_ptr, (void*)h->d_multi_loc})
    if (p) (void)hipFree(p);
  h->d_stage = nullptr, h->d_multi_ptr = h->d_multi_loc = nullptr;
  h->nmulti = int(multi_loc.size()), h->nstage = size_t(multi_ptr.back());
  if (h->nmulti > 0) {
    HIP_TRY(hipMalloc(&h->d_stage, h->nstage * sizeof(double)));
    HIP_TRY(hipMemset(h->d_stage, 0, h->nstage * sizeof(double)));
    HIP_TRY(hipMalloc(&h->d_multi_ptr, multi_ptr.size() * sizeof(int)));
    HIP_TRY(hipMalloc(&h->d_multi_loc, multi_loc.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(h->d_multi_ptr, multi_ptr.data(), multi_ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_multi_loc, multi_loc.data(), multi_loc.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  return 0;
}

int asset_hip_defect_eval_assembled_device(asset_hip_defect_t h, int what, const double* dX, const double* dL,
                                           double* d_fx_blocks, double* d_agx_blocks, double* d_kkt_values,
                                           void* stream) {
  what &= 0xff;   // (no blocks are written: ASSET_HIP_KEEP_HESSIAN_SLOTS has nothing to act on)
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (what < ASSET_HIP_JAC) return fail(ASSET_HIP_EINVAL, "assembled evaluation needs a kind that produces KKT entries");
  if (!h->d_map) return fail(ASSET_HIP_EINVAL, "no kkt map: call asset_hip_defect_set_kkt_map first");
  if (!d_kkt_values) return fail(ASSET_HIP_EINVAL, "kkt value array is null");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  // the dense stage places its accumulators in the value array itself (defect_kernels.h, ASM instantiations)
  return launch(h, what, dX, dL, d_fx_blocks, d_agx_blocks, nullptr, st, d_kkt_values);
}

// CSR by target row over the entries of a block array ([nseg][width], entry e = V * width + i goes to row index[e]):
// rows sorted ascending, short rows (<= 64 contributors) first.  Returns the split point.
static int build_rhs_csr(const std::vector<int32_t>& index, std::vector<int>& rows, std::vector<int>& ptr,
                         std::vector<int>& src) {
  const size_t n = index.size();
  std::vector<int> order(n);
  for (size_t e = 0; e < n; e++) order[e] = int(e);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return index[a] < index[b]; });   // source order within a row
  struct Row { int row, begin, end; };
  std::vector<Row> rr;
  for (size_t k = 0; k < n;) {
    size_t e = k;
    while (e < n && index[order[e]] == index[order[k]]) e++;
    rr.push_back(Row{index[order[k]], int(k), int(e)});
    k = e;
  }
  std::stable_partition(rr.begin(), rr.end(), [](const Row& r) { return r.end - r.begin <= 64; });
  rows.clear(), ptr.assign(1, 0), src.clear();
  src.reserve(n);
  int long_from = int(rr.size());
  for (size_t i = 0; i < rr.size(); i++) {
    if (rr[i].end - rr[i].begin > 64 && long_from == int(rr.size())) long_from = int(i);
    rows.push_back(rr[i].row);
    for (int k = rr[i].begin; k < rr[i].end; k++) src.push_back(order[k]);
    ptr.push_back(int(src.size()));
  }
  return long_from;
}

int asset_hip_defect_eval_kkt_device(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* d_FXE,
                                     double* d_AGX, double* d_kkt_values, void* stream) {
  what &= 0xff;   // (no blocks are written: ASSET_HIP_KEEP_HESSIAN_SLOTS has nothing to act on)
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (!d_FXE) return fail(ASSET_HIP_EINVAL, "FXE is null");
  const bool want_kkt = what >= ASSET_HIP_JAC;
  const bool want_agx = (what == ASSET_HIP_CON_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD || what == ASSET_HIP_JAC_ADJGRAD_HESS);
  if (want_kkt && (!h->d_map || !d_kkt_values)) return fail(ASSET_HIP_EINVAL, "no kkt map / value array for a kind that fills the matrix");
  if (want_agx && !d_AGX) return fail(ASSET_HIP_EINVAL, "AGX is null for a kind that produces the adjoint gradient");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : h->stream;
  const int IR = h->ke->ir, OR = h->ke->orr;
  if (!h->rhs_tables_ready) {   // the gather tables, once per handle: built into locals, committed only when all of them exist
    int* d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double *fxb = nullptr, *agxb = nullptr;
    int n_fx = 0, n_gx = 0, fx_long = 0, gx_long = 0;
    auto build = [&]() -> hipError_t {
      std::vector<int> rows, ptr, src;
      auto up = [&](int*& dst, const std::vector<int>& v) -> hipError_t {
        hipError_t e = hipMalloc(&dst, (v.size() + 1) * sizeof(int));
        return e != hipSuccess ? e : hipMemcpy(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice);
      };
      hipError_t e;
      fx_long = build_rhs_csr(h->h_cindex, rows, ptr, src);
      n_fx = int(rows.size());
      if ((e = up(d[0], rows)) != hipSuccess || (e = up(d[1], ptr)) != hipSuccess || (e = up(d[2], src)) != hipSuccess) return e;
      gx_long = build_rhs_csr(h->h_vindex, rows, ptr, src);
      n_gx = int(rows.size());
      if ((e = up(d[3], rows)) != hipSuccess || (e = up(d[4], ptr)) != hipSuccess || (e = up(d[5], src)) != hipSuccess) return e;
      if ((e = hipMalloc(&fxb, sizeof(double) * size_t(h->nseg) * OR)) != hipSuccess) return e;
      return hipMalloc(&agxb, sizeof(double) * size_t(h->nseg) * IR);
    };
    const hipError_t e = build();
    if (e != hipSuccess) {   // nothing of a half-built set stays on the handle: the next call starts over
      for (int* p : d) if (p) hipFree(p);
      if (fxb) hipFree(fxb);
      if (agxb) hipFree(agxb);
      return hipfail(e, "building the RHS gather tables");
    }
    h->d_fx_rows = d[0], h->d_fx_ptr = d[1], h->d_fx_src = d[2], h->d_gx_rows = d[3], h->d_gx_ptr = d[4], h->d_gx_src = d[5];
    h->d_fxb = fxb, h->d_agxb = agxb;
    h->n_fx_rows = n_fx, h->fx_long_from = fx_long, h->n_gx_rows = n_gx, h->gx_long_from = gx_long;
    h->rhs_tables_ready = true;
  }
  int rc = launch(h, what, dX, dL, h->d_fxb, want_agx ? h->d_agxb : nullptr, nullptr, st, want_kkt ? d_kkt_values : nullptr);
  if (rc) return rc;
  auto gather = [&](double* target, const double* blocks, const int* rows, const int* ptr, const int* src, int nrows,
                    int long_from) -> hipError_t {
    if (long_from > 0)
      hipLaunchKernelGGL(asset_hip::rhs_gather_kernel, dim3((long_from + 255) / 256), dim3(256), 0, st, target, blocks, rows, ptr,
                         src, nrows, long_from);
    if (nrows > long_from)
      hipLaunchKernelGGL(asset_hip::rhs_gather_long_kernel, dim3(nrows - long_from), dim3(256), 0, st, target, blocks, rows,
                         ptr, src, long_from);
    return hipGetLastError();
  };
  HIP_TRY(gather(d_FXE, h->d_fxb, h->d_fx_rows, h->d_fx_ptr, h->d_fx_src, h->n_fx_rows, h->fx_long_from));
  if (want_agx) HIP_TRY(gather(d_AGX, h->d_agxb, h->d_gx_rows, h->d_gx_ptr, h->d_gx_src, h->n_gx_rows, h->gx_long_from));
  return 0;
}

static int eval_assembled_host(asset_hip_defect_t h, int what, const double* X, const double* L, double* fx_blocks,
                               double* agx_blocks, double* kkt_values, bool target_zeroed);

int asset_hip_defect_eval_assembled(asset_hip_defect_t h, int what, const double* X, const double* L,
                                    double* fx_blocks, double* agx_blocks, double* kkt_values) {
  return eval_assembled_host(h, what, X, L, fx_blocks, agx_blocks, kkt_values, false);
}
int asset_hip_defect_eval_assembled_zeroed(asset_hip_defect_t h, int what, const double* X, const double* L,
                                           double* fx_blocks, double* agx_blocks, double* kkt_values) {
  return eval_assembled_host(h, what, X, L, fx_blocks, agx_blocks, kkt_values, true);
}

static int eval_assembled_host(asset_hip_defect_t h, int what, const double* X, const double* L, double* fx_blocks,
                               double* agx_blocks, double* kkt_values, bool target_zeroed) {
  what &= 0xff;
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (!X || !kkt_values) return fail(ASSET_HIP_EINVAL, "X / kkt value array is null");
  if (what < ASSET_HIP_JAC) return fail(ASSET_HIP_EINVAL, "assembled evaluation needs a kind that produces KKT entries");
  if (!h->d_map) return fail(ASSET_HIP_EINVAL, "no kkt map: call asset_hip_defect_set_kkt_map first");
  HIP_TRY(hipSetDevice(h->device));
  const size_t nfx = size_t(h->nseg) * h->ke->orr, nagx = size_t(h->nseg) * h->ke->ir;
  const size_t nval = size_t(h->value_hi - h->value_lo);
  if (!h->d_X) HIP_TRY(hipMalloc(&h->d_X, sizeof(double) * h->cap_primal));
  if (!h->d_L) HIP_TRY(hipMalloc(&h->d_L, sizeof(double) * h->cap_equal));
  if (fx_blocks && !h->d_fx) HIP_TRY(hipMalloc(&h->d_fx, sizeof(double) * size_t(h->cap_seg) * h->ke->orr));
  if (agx_blocks && !h->d_agx) HIP_TRY(hipMalloc(&h->d_agx, sizeof(double) * size_t(h->cap_seg) * h->ke->ir));
  if (!h->d_values) {
    HIP_TRY(hipMalloc(&h->d_values, sizeof(double) * nval));
    HIP_TRY(hipHostMalloc(&h->h_values, sizeof(double) * nval, hipHostMallocDefault));
  }
  HIP_TRY(hipMemcpyAsync(h->d_X, X, sizeof(double) * h->n_primal, hipMemcpyHostToDevice, h->stream));
  if (L) HIP_TRY(hipMemcpyAsync(h->d_L, L, sizeof(double) * h->n_equal, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemsetAsync(h->d_values, 0, sizeof(double) * nval, h->stream));
  // The device array covers [value_lo, value_hi) of the caller's: bias the base address so that locations index it
  // directly (integer arithmetic: the biased address is only ever used with offsets >= value_lo).
  double* biased = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(h->d_values) -
                                             uintptr_t(h->value_lo) * sizeof(double));
  int rc = asset_hip_defect_eval_assembled_device(h, what, h->d_X, L ? h->d_L : nullptr, fx_blocks ? h->d_fx : nullptr,
                                                  agx_blocks ? h->d_agx : nullptr, biased, h->stream);
  if (rc) return rc;
  if (fx_blocks) HIP_TRY(hipMemcpyAsync(fx_blocks, h->d_fx, sizeof(double) * nfx, hipMemcpyDeviceToHost, h->stream));
  if (agx_blocks && what != ASSET_HIP_JAC)
    HIP_TRY(hipMemcpyAsync(agx_blocks, h->d_agx, sizeof(double) * nagx, hipMemcpyDeviceToHost, h->stream));
  if (target_zeroed) {
    // the caller's range holds zeros (it was just cleared and this constraint is the first to fill it): the values go
    // straight into it -- by DMA when the array is page-locked (asset_hip_host_register), through the driver's staging
    // otherwise -- and no host pass over the values is needed at all
    HIP_TRY(hipMemcpyAsync(kkt_values + h->value_lo, h->d_values, sizeof(double) * nval, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(h->h_values, h->d_values, sizeof(double) * nval, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  // accumulate, as the reference's fill does: O(nnz) contiguous adds, split over a few threads (memory-bound)
  double* dst = kkt_values + h->value_lo;
  const double* src = h->h_values;
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nthr = nval < (size_t(1) << 18) ? 1 : (hw >= 8 ? 8 : (hw ? hw : 1));
  auto add = [=](size_t b, size_t e) { for (size_t i = b; i < e; i++) dst[i] += src[i]; };
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nthr; t++) pool.emplace_back(add, nval * t / nthr, nval * (t + 1) / nthr);
  add(0, nval / nthr);
  for (auto& th : pool) th.join();
  return 0;
}

}  // extern "C"

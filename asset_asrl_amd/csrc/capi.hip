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
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/asset_hip.h"
#include <dlfcn.h>
#include <elf.h>
#include <unistd.h>

#include "registry.h"
#include "propagate_event_kernels.h"
#include "propagate_event_stm_kernels.h"
#include "propagate_ctrl_kernels.h"
#include "capi/arena.h"
#include "capi/kkt_map.h"
#include "capi/owners.h"
#include "capi/propagate_plan.h"

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
#define HIP_TRY_AS(expr, where)                           \
  do {                                                    \
    hipError_t _e = (expr);                               \
    if (_e != hipSuccess) return hipfail(_e, where);      \
  } while (0)
#define HIP_TRY(expr) HIP_TRY_AS(expr, #expr)

using asset_hip::DeviceBuffer;
using asset_hip::PinnedBuffer;
using asset_hip::stream_or;
using asset_hip::use_device;
using asset_hip::wants_kkt;
using asset_hip::wants_multipliers;

// v on the device, in a buffer of v.size() + pad elements
template <class T>
hipError_t upload(DeviceBuffer<T>& dst, const std::vector<T>& v, size_t pad = 0) {
  const hipError_t e = dst.allocate(v.size() + pad);
  return e != hipSuccess ? e : hipMemcpy(dst.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

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

// Members are grouped by what invalidates them: a group is dropped by assigning an empty one, and a new one is built in a local and
// committed by one move.  The stream and the events come first, so they go last: buffers, then events, then the stream.
struct asset_hip_defect {
  const asset_hip::KernelEntry* ke = nullptr;
  int nseg = 0, n_primal = 0, n_equal = 0, device = 0;
  int cus = 256;
  int bundles = 0;                   // bundles that hold this handle (asset_hip_bundle_create)
  bool destroy_pending = false;      // asset_hip_defect_destroy was called while a bundle held it: freed with the last bundle
  asset_hip::Stream stream;
  asset_hip::Event ev0, ev1;
  // the caller's stream of the last *_device entry point (asset_hip_defect_rebind drains it before it touches the tables those
  // launches read: a torch side stream or hipStreamLegacy is not ordered with the handle's own stream)
  hipStream_t last_stream = nullptr;
  bool last_stream_used = false;
  // what the buffers below were sized for (asset_hip_defect_rebind keeps them while the new mesh fits)
  int cap_seg = 0, cap_primal = 0, cap_equal = 0;
  struct MeshTables {
    DeviceBuffer<int> vindex, cindex;
    DeviceBuffer<double> work;                        // per-workgroup ODE result slots
    int affine = 0, aff_v0 = 0, aff_vs = 0, aff_c0 = 0, aff_cs = 0;   // index rows that are runs (EvalArgs::affine)
    std::vector<int32_t> h_vindex, h_cindex;          // kept for the RHS tables (built on first use)
  } mesh;
  struct HostStaging {   // of the host-pointer entry points (allocated lazily, for the capacities above)
    DeviceBuffer<double> X, L, fx, agx, kkt;
  } staging;
  struct DeviceKktMap {  // on-device KKT assembly (asset_hip_defect_set_kkt_map); no map words: no map
    DeviceBuffer<int32_t> map;                        // value location of every accumulator entry, fragment order (defect_kernels.h, ASM)
    // locations with three or more contributing slots: staged cells + fixed-order reduction (defect_dims.h, asm_reduce_kernel)
    DeviceBuffer<double> stage;
    DeviceBuffer<int32_t> multi_ptr, multi_loc;
    long long value_lo = 0, value_hi = 0, nvalues = 0;
    DeviceBuffer<double> d_values;                    // [value_hi - value_lo) staging for the host-pointer entry point
    PinnedBuffer<double> h_values;                    // pinned mirror of d_values
  } kmap;
  struct RhsTables {     // device RHS fill (asset_hip_defect_eval_kkt_device): CSR by target row over the FX / AGX block entries
    DeviceBuffer<int> fx_rows, fx_ptr, fx_src, gx_rows, gx_ptr, gx_src;
    int n_fx_rows = 0, fx_long_from = 0, n_gx_rows = 0, gx_long_from = 0;
    DeviceBuffer<double> fxb, agxb;                   // block buffers of that entry point; agxb is the last to be built
  } rhs;
  DeviceBuffer<double> aconst;     // constants of every application of a plain function (asset_hip_defect_set_appl_consts)
  DeviceBuffer<char> lane[3];      // per-lane constants of the dense stage by derivative level
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

// The meta table of a module (rtc_device.h: asset_rtc_meta) read from the code object itself, on the host: the symbol's section and
// offset in the ELF image.  Modules of kind 4 are registered this way, without a device (their launch loads them where it runs).
bool rtc_meta_from_code(const std::vector<char>& code, long long* meta) {
  static const char magic[4] = {0x7f, 'E', 'L', 'F'};
  const auto it = std::search(code.begin(), code.end(), magic, magic + 4);   // (a bundled code object carries the image behind a header)
  if (it == code.end()) return false;
  const char* base = code.data() + (it - code.begin());
  const size_t size = size_t(code.end() - it);
  Elf64_Ehdr eh;
  if (size < sizeof eh) return false;
  std::memcpy(&eh, base, sizeof eh);
  if (eh.e_ident[EI_CLASS] != ELFCLASS64 || eh.e_shentsize != sizeof(Elf64_Shdr) || eh.e_shoff > size ||
      size_t(eh.e_shnum) * sizeof(Elf64_Shdr) > size - eh.e_shoff)
    return false;
  std::vector<Elf64_Shdr> sh(eh.e_shnum);
  if (!sh.empty()) std::memcpy(sh.data(), base + eh.e_shoff, sh.size() * sizeof(Elf64_Shdr));
  auto inside = [&](const Elf64_Shdr& h) { return h.sh_offset <= size && h.sh_size <= size - h.sh_offset; };
  static const char want[] = "asset_rtc_meta";
  const size_t bytes = sizeof(long long) * asset_hip::MF_COUNT;
  for (const Elf64_Shdr& st : sh) {
    if ((st.sh_type != SHT_SYMTAB && st.sh_type != SHT_DYNSYM) || st.sh_entsize != sizeof(Elf64_Sym) || !inside(st) || st.sh_link >= sh.size())
      continue;
    const Elf64_Shdr& str = sh[st.sh_link];
    if (!inside(str)) continue;
    for (size_t k = 0; k < st.sh_size / sizeof(Elf64_Sym); k++) {
      Elf64_Sym sym;
      std::memcpy(&sym, base + st.sh_offset + k * sizeof sym, sizeof sym);
      if (sym.st_name >= str.sh_size || str.sh_size - sym.st_name < sizeof want ||
          std::memcmp(base + str.sh_offset + sym.st_name, want, sizeof want) != 0)
        continue;
      if (sym.st_shndx >= sh.size() || sym.st_size != bytes) return false;
      const Elf64_Shdr& sec = sh[sym.st_shndx];
      if (sec.sh_type == SHT_NOBITS || !inside(sec) || sym.st_value < sec.sh_addr || sym.st_value - sec.sh_addr > sec.sh_size ||
          sec.sh_size - (sym.st_value - sec.sh_addr) < bytes)
        return false;
      std::memcpy(meta, base + sec.sh_offset + (sym.st_value - sec.sh_addr), bytes);
      return true;
    }
  }
  return false;
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
  if (!source || !functor || !cache_path || kind < 1 || kind > 6) return fail(ASSET_HIP_EINVAL, "bad jit arguments");
  RtcBlob blob;
  const int rc = rtc_compile(source, functor, kind, mode, blocked, seg_per_group, options, noptions, blob);
  if (rc) return rc;
  if (!rtc_write(cache_path, blob)) return fail(ASSET_HIP_EINVAL, std::string("cannot write ") + cache_path);
  return 0;
}

int asset_hip_jit_plugin(const char* name, const char* source, const char* functor, int kind, int mode, int blocked,
                         int seg_per_group, const char* const* options, int noptions, const char* cache_path) {
  if (!name || !functor || kind < 1 || kind > 6) return fail(ASSET_HIP_EINVAL, "bad jit arguments");
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
  std::unique_ptr<asset_hip::KernelTable> table(new asset_hip::KernelTable());
  if (kind >= 4) {
    // an ODE with event functions, or with a control law: the table comes from the code object on the host, so that asset_hip_propagate_events can check
    // its arguments against it before a device is touched; the module is loaded by its first launch
    if (!rtc_meta_from_code(rtc->code, table->meta))
      return fail(ASSET_HIP_ECOMPILE, "the module has no asset_rtc_meta table of the expected size (rtc_device.h)");
  } else {
    hipModule_t mod = nullptr;
    hipError_t e = rtc->module_on_current_device(&mod);
    if (e != hipSuccess) return hipfail(e, "loading the run-time module (hipModuleLoadData / hipModuleGetFunction)");
    hipDeviceptr_t dmeta = nullptr;
    size_t mbytes = 0;
    e = hipModuleGetGlobal(&dmeta, &mbytes, mod, "asset_rtc_meta");
    if (e != hipSuccess || mbytes != sizeof table->meta)
      return fail(ASSET_HIP_ECOMPILE, "the module has no asset_rtc_meta table of the expected size (rtc_device.h)");
    if ((e = hipMemcpy(table->meta, reinterpret_cast<void*>(dmeta), sizeof table->meta, hipMemcpyDeviceToHost)) != hipSuccess)
      return hipfail(e, "reading asset_rtc_meta");
  }
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

// The meta table of a cached module file, read on the host as asset_hip_jit_plugin reads it for kind 4 (rtc_meta_from_code): for
// tools and tests -- a file that is cut short or damaged is an error, never a crash.  Returns MF_COUNT.
int asset_hip_rtc_module_meta(const char* cache_path, long long* meta, int cap) {
  if (!cache_path || !meta) return fail(ASSET_HIP_EINVAL, "null argument");
  if (cap < asset_hip::MF_COUNT) return fail(ASSET_HIP_EINVAL, "output buffer too small");
  RtcBlob blob;
  if (!rtc_read(cache_path, blob)) return fail(ASSET_HIP_EINVAL, std::string("no compiled module at ") + cache_path);
  long long tmp[asset_hip::MF_COUNT];
  if (!rtc_meta_from_code(blob.code, tmp)) return fail(ASSET_HIP_EINVAL, "the code object holds no readable asset_rtc_meta table");
  for (int k = 0; k < asset_hip::MF_COUNT; k++) meta[k] = tmp[k];
  return asset_hip::MF_COUNT;
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
  const bool trap = !std::strcmp(which, "mesh_trapezoidal");
  if (trap || !std::strcmp(which, "mesh")) {   // the estimator's scheme (mesh_kernels.h): order, error weight, factorial, xw[cs], dxw[cs]
    if (trap && cs != 2) return fail(ASSET_HIP_EINVAL, "the Trapezoidal scheme has two nodes");
    const asset_hip::MeshScheme sc = asset_hip::mesh_scheme(trap ? 1 : cs);   // (LGL modes carry their cs as the mode number)
    if (cap < 3 + 2 * cs) return fail(ASSET_HIP_EINVAL, "output buffer too small");
    out[0] = sc.order, out[1] = sc.error_weight, out[2] = sc.factorial;
    for (int j = 0; j < cs; j++) out[3 + j] = sc.xw[j], out[3 + cs + j] = sc.dxw[j];
    return 3 + 2 * cs;
  }
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

// The kernels trust the index tables: every entry names a row of the solver vector / of the equality constraints
static int check_index_tables(const asset_hip::KernelEntry* ke, int nseg, const int32_t* vindex, const int32_t* cindex, int n_primal,
                              int n_equal) {
  const size_t nv = size_t(ke->ir) * nseg, nc = size_t(ke->orr) * nseg;
  for (size_t i = 0; i < nv; i++)
    if (vindex[i] < 0 || vindex[i] >= n_primal) return fail(ASSET_HIP_ERANGE, "vindex entry out of range");
  for (size_t i = 0; i < nc; i++)
    if (cindex[i] < 0 || cindex[i] >= n_equal) return fail(ASSET_HIP_ERANGE, "cindex entry out of range");
  return 0;
}

// Index tables of a handle (checked by the caller: check_index_tables): upload, run detection; buffers that depend on the number of
// applications are kept while they fit and re-allocated otherwise; everything derived from the OLD tables is dropped.
static int bind_tables(asset_hip_defect_t h, int nseg, const int32_t* vindex, const int32_t* cindex, int n_primal, int n_equal) {
  const asset_hip::KernelEntry* ke = h->ke;
  const size_t nv = size_t(ke->ir) * nseg, nc = size_t(ke->orr) * nseg;
  if (h->stream.get()) HIP_TRY(hipStreamSynchronize(h->stream.get()));   // (nothing of the old mesh is in flight on the handle's own stream ...
  if (h->last_stream_used) {                                     //  ... nor on the caller's stream of the last *_device call;
    if (hipStreamSynchronize(h->last_stream) != hipSuccess) (void)hipGetLastError();   //  a stream the caller has destroyed since is drained)
    h->last_stream_used = false;
  }
  // FAILURE-ATOMIC: every new buffer is allocated and filled through locals; the handle is touched only once all of that has succeeded.
  // A failed re-bind (out of device memory on a grown mesh) leaves the handle exactly as it was -- old mesh, old tables, still usable.
  DeviceBuffer<int> nvi, nci;
  DeviceBuffer<double> nwork;
  int cap = h->cap_seg;
  const bool grow = nseg > h->cap_seg;
  if (grow) {                                                    // grow: index tables, workspace, block staging
    cap = h->cap_seg > 0 ? std::max(nseg, h->cap_seg + h->cap_seg / 4) : nseg;   // (re-meshing grows by steps)
    HIP_TRY_AS(nvi.allocate(size_t(ke->ir) * cap), "hipMalloc(vindex)");
    HIP_TRY_AS(nci.allocate(size_t(ke->orr) * cap), "hipMalloc(cindex)");
    if (ke->work_doubles) {
      HIP_TRY_AS(nwork.allocate(size_t(cap) * ke->work_doubles), "hipMalloc(workspace)");
      // sections no kernel writes must read as zero (the interior-point sections of a Trapezoidal slot, defect_dims.h)
      HIP_TRY_AS(hipMemset(nwork.get(), 0, size_t(cap) * ke->work_doubles * sizeof(double)), "hipMemset(workspace)");
    }
  }
  // (when the mesh still fits the kept tables are overwritten in place: both streams were drained above, and a failed copy into them
  //  poisons the handle -- nseg = 0 -- instead of leaving half-written tables behind an old segment count)
  hipError_t e;
  if ((e = hipMemcpy(grow ? nvi.get() : h->mesh.vindex.get(), vindex, nv * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) {
    if (!grow) h->nseg = 0;
    return hipfail(e, "hipMemcpy(vindex)");
  }
  if ((e = hipMemcpy(grow ? nci.get() : h->mesh.cindex.get(), cindex, nc * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) {
    if (!grow) h->nseg = 0;
    return hipfail(e, "hipMemcpy(cindex)");
  }
  if (grow) {
    h->mesh.vindex = std::move(nvi), h->mesh.cindex = std::move(nci), h->mesh.work = std::move(nwork), h->cap_seg = cap;
    h->staging.fx = {}, h->staging.agx = {}, h->staging.kkt = {};
  }
  if (n_primal > h->cap_primal) h->staging.X = {}, h->cap_primal = n_primal;
  if (n_equal > h->cap_equal) h->staging.L = {}, h->cap_equal = n_equal;
  asset_hip_defect::MeshTables& m = h->mesh;
  m.h_vindex.assign(vindex, vindex + nv);
  m.h_cindex.assign(cindex, cindex + nc);
  {   // rows that are runs with a constant stride between applications (EvalArgs::affine)
    const int ir = ke->ir, orr = ke->orr, ns = nseg;
    const int v0 = vindex[0], c0 = cindex[0];
    const int vs = ns > 1 ? vindex[ir] - v0 : 0, cs = ns > 1 ? cindex[orr] - c0 : 0;
    bool ok = true;
    for (int s = 0; s < ns && ok; s++) {
      for (int k = 0; k < ir && ok; k++) ok = vindex[size_t(s) * ir + k] == v0 + s * vs + k;
      for (int k = 0; k < orr && ok; k++) ok = cindex[size_t(s) * orr + k] == c0 + s * cs + k;
    }
    m.affine = ok ? 1 : 0, m.aff_v0 = v0, m.aff_vs = vs, m.aff_c0 = c0, m.aff_cs = cs;
  }
  // derived from the old tables: the KKT map and its staging, the RHS gather tables and block buffers, per-application constants
  h->kmap = {}, h->rhs = {}, h->aconst = {};
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
  if (ke->table->meta[asset_hip::MF_KIND] == 4)
    return fail(ASSET_HIP_EINVAL, "an event module is launched through asset_hip_propagate_events, it is not a function");
  if (ke->table->meta[asset_hip::MF_KIND] == 5)
    return fail(ASSET_HIP_EINVAL, "a controller module is launched through asset_hip_propagate_ctrl*, it is not a function");
  if (ke->table->meta[asset_hip::MF_KIND] == 6)
    return fail(ASSET_HIP_EINVAL, "an event module is launched through asset_hip_propagate_events_stm, it is not a function");
  // (before anything is allocated: the commonest set-up error)
  if (const int rc = check_index_tables(ke, d->nseg, d->vindex, d->cindex, d->n_primal, d->n_equal)) return rc;
  if (const int rc = use_device(d->device, "no HIP device visible: the evaluator has no CPU fallback")) return rc;
  // (a failing path below returns: the handle goes as asset_hip_defect_destroy lets it go)
  std::unique_ptr<asset_hip_defect, void (*)(asset_hip_defect_t)> h(new (std::nothrow) asset_hip_defect, asset_hip_defect_destroy);
  if (!h) return fail(ASSET_HIP_EINVAL, "out of host memory");
  h->ke = ke, h->device = d->device;
  hipDeviceProp_t prop;
  const hipError_t e = hipGetDeviceProperties(&prop, d->device);
  h->cus = (e == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  HIP_TRY_AS(h->stream.create(), "hipStreamCreate");
  if (const int rc = bind_tables(h.get(), d->nseg, d->vindex, d->cindex, d->n_primal, d->n_equal)) return rc;
  // per-lane constants of the dense stage: computed here, once
  for (int level = 0; level <= 2; level++) {   // (0: the record of the resident kernel)
    const size_t nb = asset_hip::entry_lane_bytes(ke, level);
    if (!nb) continue;
    // ASSET_LANE_REPLICAS copies: every workgroup of the dense stage loads the whole table when it starts, all at the
    // same moment -- with one copy that is thousands of requests for the same few hundred cache lines, which the L2
    // channels holding them serve one after the other; workgroup b reads copy b % ASSET_LANE_REPLICAS.
    HIP_TRY_AS(h->lane[level].allocate(nb * ASSET_LANE_REPLICAS), "hipMalloc(lane constants)");
    char* lane = h->lane[level].get();
    HIP_TRY_AS(asset_hip::entry_lane_setup(ke, level, lane, h->stream.get()), "lane_setup_kernel");
    for (int r = 1; r < ASSET_LANE_REPLICAS; r++)
      HIP_TRY_AS(hipMemcpyAsync(lane + size_t(r) * nb, lane, nb, hipMemcpyDeviceToDevice, h->stream.get()), "hipMemcpy(lane constants)");
  }
  HIP_TRY_AS(hipStreamSynchronize(h->stream.get()), "lane_setup_kernel");
  HIP_TRY_AS(h->ev0.create(), "hipEventCreate");
  HIP_TRY_AS(h->ev1.create(), "hipEventCreate");
  *out = h.release();
  return 0;
}

int asset_hip_defect_rebind(asset_hip_defect_t h, int nseg, const int32_t* vindex, const int32_t* cindex, int n_primal, int n_equal) {
  if (!h || !vindex || !cindex || nseg <= 0 || n_primal <= 0 || n_equal <= 0) return fail(ASSET_HIP_EINVAL, "bad rebind arguments");
  if (h->bundles > 0) return fail(ASSET_HIP_EINVAL, "the handle is a member of a bundle: destroy the bundle before re-binding");
  HIP_TRY(hipSetDevice(h->device));
  if (const int rc = check_index_tables(h->ke, nseg, vindex, cindex, n_primal, n_equal)) return rc;
  return bind_tables(h, nseg, vindex, cindex, n_primal, n_equal);
}

void asset_hip_defect_destroy(asset_hip_defect_t h) {
  if (!h) return;
  if (h->bundles > 0) {   // a bundle launches through this handle's tables and buffers: it lives until that bundle is gone
    h->destroy_pending = true;
    return;
  }
  (void)hipSetDevice(h->device);
  if (h->stream.get()) (void)hipStreamSynchronize(h->stream.get());
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
  if (ke->table->meta[asset_hip::MF_KIND] == 4)
    return fail(ASSET_HIP_EINVAL, "an event module is launched through asset_hip_propagate_events, it is not a function");
  if (ke->table->meta[asset_hip::MF_KIND] == 5)
    return fail(ASSET_HIP_EINVAL, "a controller module is launched through asset_hip_propagate_ctrl*, it is not a function");
  if (ke->table->meta[asset_hip::MF_KIND] == 6)
    return fail(ASSET_HIP_EINVAL, "an event module is launched through asset_hip_propagate_events_stm, it is not a function");
  if (nkkt) *nkkt = ke->nkkt;
  return entry_kkt_layout(ke, stride, rows, cols);
}

// The launch plan (registry.h: plan_lgl) of one evaluation kind, with the default dispatch -- what a handle of `nseg` segments on
// a device of `cus` compute units launches when no tuning knob is in effect.  `functions`: the handle of a plain function is
// answered with its one launch (registry.h: plan_func); the query by name is for the transcriptions of an ODE only
static int entry_launch_plan(const asset_hip::KernelEntry* ke, int what, int assembled, int nseg, int cus, bool res_record,
                             asset_hip_launch_plan* out, bool functions = false) {
  const int level = level_of(what);
  if (!out || level < 0 || (what & ~0xff) || (assembled && what < ASSET_HIP_JAC)) return fail(ASSET_HIP_EINVAL, "bad launch plan query");
  if (ke->table->meta[asset_hip::MF_KIND] == 2 && functions) {   // a plain function: one launch (registry.h: plan_func)
    if (nseg < 1) return fail(ASSET_HIP_EINVAL, "bad launch plan query (nseg and cus are positive)");
    const asset_hip::FuncPlan f = asset_hip::plan_func(ke->table->meta, level, assembled != 0, nseg);
    if (!ke->table->k[f.slot]) return fail(ASSET_HIP_ENOODE, std::string("the plan names a kernel this function lacks: ") + asset_hip::kslot_name(f.slot));
    *out = asset_hip_launch_plan();
    out->nsteps = 1;
    out->step[0] = asset_hip_plan_step{f.slot, int(f.grid), 1, 64, (long long)f.lds_bytes, asset_hip::PLAN_NO_EXTRA, f.apw};
    return 0;
  }
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
  if (ke->table->meta[asset_hip::MF_KIND] == 4)
    return fail(ASSET_HIP_EINVAL, "an event module is launched through asset_hip_propagate_events, it is not a function");
  if (ke->table->meta[asset_hip::MF_KIND] == 5)
    return fail(ASSET_HIP_EINVAL, "a controller module is launched through asset_hip_propagate_ctrl*, it is not a function");
  if (ke->table->meta[asset_hip::MF_KIND] == 6)
    return fail(ASSET_HIP_EINVAL, "an event module is launched through asset_hip_propagate_events_stm, it is not a function");
  return entry_launch_plan(ke, what, assembled, nseg, cus, asset_hip::entry_lane_bytes(ke, 0) > 0, out);
}
int asset_hip_defect_launch_plan(asset_hip_defect_t h, int what, int assembled, asset_hip_launch_plan* out) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  return entry_launch_plan(h->ke, what, assembled, h->nseg, h->cus, bool(h->lane[0]), out, true);
}
const char* asset_hip_kernel_slot_name(int slot) { return asset_hip::kslot_name(slot); }
int asset_hip_kernel_slot_kinds(int slot) {
  int kinds = 0;
  for (int kind = 1; kind <= 6; kind++)
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
  const bool needs_l = wants_multipliers(what);
  if (needs_l && !dL) return fail(ASSET_HIP_EINVAL, "L is null for an evaluation kind that contracts with multipliers");
  a.nseg = h->nseg;
  a.X = dX;
  a.L = needs_l ? dL : nullptr;
  const asset_hip_defect::MeshTables& m = h->mesh;
  a.vindex = m.vindex.get();
  a.cindex = m.cindex.get();
  a.FX = dfx;
  a.AGX = needs_l ? dagx : nullptr;
  a.KKT = wants_kkt(what) ? dkkt : nullptr;
  a.work = m.work.get();
  a.lane_consts = level >= 1 ? h->lane[level].get() : nullptr;
  a.lane_consts_res = h->lane[0].get();
  a.affine = asset_hip::tuning().no_affine ? 0 : m.affine, a.aff_v0 = m.aff_v0, a.aff_vs = m.aff_vs, a.aff_c0 = m.aff_c0, a.aff_cs = m.aff_cs;
  a.appl_consts = h->aconst.get();
  if (h->ke->naconst > 0 && !h->aconst)
    return fail(ASSET_HIP_EINVAL, "this function reads constants of its applications: call asset_hip_defect_set_appl_consts first");
  return 0;
}

static int launch(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx, double* dagx,
                  double* dkkt, hipStream_t st, double* d_values = nullptr) {
  if (st != h->stream.get()) h->last_stream = st, h->last_stream_used = true;
  asset_hip::EvalArgs a;
  const int rc = fill_args(h, what, dX, dL, dfx, dagx, dkkt, a);
  if (rc) return rc;
  const int level = level_of(what);
  if (d_values) {                                                          // on-device assembly
    a.kmap = h->kmap.map.get(), a.values = d_values, a.KKT = nullptr;
    a.stage = h->kmap.stage.get(), a.nvalues = int(h->kmap.nvalues);
  }
  hipError_t e = asset_hip::entry_launch(h->ke, level, a, h->cus, st);
  if (e != hipSuccess) return hipfail(e, "kernel launch");
  if (d_values && h->kmap.multi_loc && level >= 2) {   // the staged locations (Hessian entries only): fixed-order sums
    hipLaunchKernelGGL(asset_hip::asm_reduce_kernel, dim3(unsigned(h->kmap.multi_loc.size())), dim3(256), 0, st, d_values, h->kmap.stage.get(),
                       h->kmap.multi_ptr.get(), h->kmap.multi_loc.get());
    if ((e = hipGetLastError()) != hipSuccess) return hipfail(e, "asm_reduce_kernel");
  }
  return 0;
}

int asset_hip_defect_eval_device(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx,
                                 double* dagx, double* dkkt, void* stream) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  HIP_TRY(hipSetDevice(h->device));
  return launch(h, what, dX, dL, dfx, dagx, dkkt, stream_or(h, stream));
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
    const asset_hip::FuncPlan p = asset_hip::plan_func(h->ke->table->meta, level, false, h->nseg);   // (a bundle writes blocks only)
    if (p.lds_bytes > shmem) shmem = p.lds_bytes;
    args.start[k] = blocks;
    blocks += int(p.grid);
  }
  for (int k = n; k <= asset_hip::BUNDLE_MAX; k++) args.start[k] = blocks;
  void* kargs[] = {&args};
  hipStream_t st = stream_or(b->members[0], stream);
  const int slot = level == 0 ? asset_hip::K_BUNDLE0 : (level == 1 ? asset_hip::K_BUNDLE1 : asset_hip::K_BUNDLE2);
  hipError_t e = asset_hip::klaunch(b->ke->table->k[slot], dim3(blocks), dim3(64), shmem, st, kargs);
  if (e != hipSuccess) return hipfail(e, "bundle launch");
  return 0;
}

int asset_hip_defect_time_device(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* dfx,
                                 double* dagx, double* dkkt, int warmup, int iters, float* ms_per_launch) {
  if (!h || !ms_per_launch || iters <= 0) return fail(ASSET_HIP_EINVAL, "bad timing arguments");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream.get();
  for (int i = 0; i < warmup; i++) {
    int rc = launch(h, what, dX, dL, dfx, dagx, dkkt, st);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev0.get(), st));
  for (int i = 0; i < iters; i++) {
    int rc = launch(h, what, dX, dL, dfx, dagx, dkkt, st);
    if (rc) return rc;
  }
  HIP_TRY(hipEventRecord(h->ev1.get(), st));
  HIP_TRY(hipEventSynchronize(h->ev1.get()));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev0.get(), h->ev1.get()));
  *ms_per_launch = ms / float(iters);
  return 0;
}

// The staging of the host-pointer entry points: allocated on first use, sized for the handle's capacity (asset_hip_defect_rebind
// keeps it while the new mesh fits); X and L copied in on the handle's stream
static int stage_inputs(asset_hip_defect_t h, const double* X, const double* L, bool fx, bool agx, bool kkt) {
  asset_hip_defect::HostStaging& s = h->staging;
  if (!s.X) HIP_TRY(s.X.allocate(h->cap_primal));
  if (!s.L) HIP_TRY(s.L.allocate(h->cap_equal));
  if (fx && !s.fx) HIP_TRY(s.fx.allocate(size_t(h->cap_seg) * h->ke->orr));
  if (agx && !s.agx) HIP_TRY(s.agx.allocate(size_t(h->cap_seg) * h->ke->ir));
  if (kkt && !s.kkt) HIP_TRY(s.kkt.allocate(size_t(h->cap_seg) * h->ke->kstride));
  HIP_TRY(hipMemcpyAsync(s.X.get(), X, sizeof(double) * h->n_primal, hipMemcpyHostToDevice, h->stream.get()));
  if (L) HIP_TRY(hipMemcpyAsync(s.L.get(), L, sizeof(double) * h->n_equal, hipMemcpyHostToDevice, h->stream.get()));
  return 0;
}

int asset_hip_defect_eval(asset_hip_defect_t h, int what, const double* X, const double* L, double* fx, double* agx,
                          double* kkt) {
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (!X) return fail(ASSET_HIP_EINVAL, "X is null");
  HIP_TRY(hipSetDevice(h->device));
  const size_t nfx = size_t(h->nseg) * h->ke->orr, nagx = size_t(h->nseg) * h->ke->ir,
               nkkt = size_t(h->nseg) * h->ke->kstride;   // (blocks in the handle's layout: asset_hip_defect_kkt_layout)
  int rc = stage_inputs(h, X, L, fx, agx, kkt);
  if (rc) return rc;
  const asset_hip_defect::HostStaging& s = h->staging;
  hipStream_t st = h->stream.get();
  rc = launch(h, what, s.X.get(), L ? s.L.get() : nullptr, fx ? s.fx.get() : nullptr, agx ? s.agx.get() : nullptr,
              kkt ? s.kkt.get() : nullptr, st);
  if (rc) return rc;
  const int level = level_of(what);
  if (fx) HIP_TRY(hipMemcpyAsync(fx, s.fx.get(), sizeof(double) * nfx, hipMemcpyDeviceToHost, st));
  if (agx && wants_multipliers(what)) HIP_TRY(hipMemcpyAsync(agx, s.agx.get(), sizeof(double) * nagx, hipMemcpyDeviceToHost, st));
  if (kkt && level >= 1 && wants_kkt(what)) HIP_TRY(hipMemcpyAsync(kkt, s.kkt.get(), sizeof(double) * nkkt, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

int asset_hip_defect_set_appl_consts(asset_hip_defect_t h, const double* consts, int per_application) {
  if (!h || !consts) return fail(ASSET_HIP_EINVAL, "null handle / constants");
  if (per_application != h->ke->naconst || per_application <= 0)
    return fail(ASSET_HIP_EINVAL, "the number of constants per application does not match the function");
  HIP_TRY(hipSetDevice(h->device));
  const size_t n = size_t(h->nseg) * per_application;
  if (!h->aconst) HIP_TRY(h->aconst.allocate(n));
  HIP_TRY(hipMemcpy(h->aconst.get(), consts, n * sizeof(double), hipMemcpyHostToDevice));
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

}  // extern "C"

// ------------------------------------------------------------------------- the integrating entry points: their host side
namespace {
// the option rules of the integrating entry points; the reference's phase defaults (ODEPhase.h:49; Integrator.h:172, 297-310)
int integ_options_checked(const asset_hip_integ_options* opt, asset_hip::IntegOptions& o) {
  o = asset_hip::IntegOptions{0.01, 0.01 / 10000, 0.01 * 10000, 3.0, 1, 100000};
  if (opt) o = asset_hip::IntegOptions{opt->def_step, opt->min_step, opt->max_step, opt->max_step_change, opt->adaptive != 0, opt->max_steps};
  if (!(o.def_step > 0.0) || !(o.min_step > 0.0) || !(o.max_step > 0.0)) return fail(ASSET_HIP_EINVAL, "step sizes must be positive");
  if (o.min_step > o.def_step || o.def_step > o.max_step) return fail(ASSET_HIP_EINVAL, "step sizes must satisfy min <= def <= max");
  if (!(o.max_step_change > 0.0)) return fail(ASSET_HIP_EINVAL, "max_step_change must be positive");
  if (o.max_steps < 1) return fail(ASSET_HIP_EINVAL, "max_steps must be at least 1");
  return 0;
}

// the tolerances as the kernels read them: abs[n] | rel[n]
std::vector<double> integ_tols_packed(const asset_hip_integ_options* opt, int n) {
  std::vector<double> tols(2 * size_t(n));
  for (int k = 0; k < n; k++) {
    tols[k] = (opt && opt->abs_tols) ? opt->abs_tols[k] : 1.0e-12;
    tols[n + k] = (opt && opt->rel_tols) ? opt->rel_tols[k] : 0.0;
  }
  return tols;
}

// the reference's two checkInput errors (LGLInterpTable.h:147-165) over the times of node rows [x, t, u, p]
int traj_times_checked(const double* traj, int nnodes, int N, int n) {
  const double dirn = traj[size_t(nnodes - 1) * N + n] - traj[n];
  for (int j = 0; j + 1 < nnodes; j++) {
    const double d = traj[size_t(j + 1) * N + n] - traj[size_t(j) * N + n];
    if (d == 0.0) return fail(ASSET_HIP_EINVAL, "the trajectory holds duplicate times (node " + std::to_string(j) + ")");
    if ((d > 0.0) != (dirn > 0.0)) return fail(ASSET_HIP_EINVAL, "the trajectory's times are not monotonic (node " + std::to_string(j) + ")");
  }
  return 0;
}

// The device side of one integrating call.  Every array of the kernels' argument struct is TAKEN from one of two arenas
// (capi/arena.h: doubles, ints) with its length, once; allocate() makes the one allocation behind each arena, of the size the takes
// add up to, and points the struct's members into it.  Inputs go in and results come out as tables of rows walked by copy().
struct IntegCall {
  asset_hip::Arena<double> d;
  asset_hip::Arena<int> i;
  DeviceBuffer<double> dbuf;
  DeviceBuffer<int> ibuf;

  // `count` elements between a host array (null: the row is skipped) and its place on the device
  struct Row {
    void* host;
    const void* dev;
    size_t bytes;
    const char* label;   // hipMemcpy(label) in the error text
    template <class T>
    Row(const T* h, const T* dv, size_t count, const char* l) : host(const_cast<T*>(h)), dev(dv), bytes(count * sizeof(T)), label(l) {}
  };

  int allocate() {
    if (d.overflowed() || i.overflowed()) return fail(ASSET_HIP_EINVAL, "the arrays of the call do not fit the address space");
    HIP_TRY_AS(dbuf.allocate(d.total()), "hipMalloc(arrays)");
    if (i.total()) HIP_TRY_AS(ibuf.allocate(i.total()), "hipMalloc(arrays)");
    d.bind(dbuf.get()), i.bind(ibuf.get());
    return 0;
  }
  // the rows in order, one blocking copy each
  static int copy(const std::vector<Row>& rows, hipMemcpyKind kind) {
    for (const Row& r : rows) {
      if (!r.host) continue;
      void* dev = const_cast<void*>(r.dev);
      const bool in = kind == hipMemcpyHostToDevice;
      const hipError_t e = hipMemcpy(in ? dev : r.host, in ? r.host : dev, r.bytes, kind);
      if (e != hipSuccess) return hipfail(e, ("hipMemcpy(" + std::string(r.label) + ")").c_str());
    }
    return 0;
  }
  // the inputs: node or problem rows (traj, y0), then the final times and the tolerances abs | rel where the call has them
  static int upload(const double* d_rows, const double* rows, size_t nrows, const char* label, const double* d_abs = nullptr,
                    const asset_hip_integ_options* opt = nullptr, int n = 0, const double* d_tf = nullptr, const double* tf = nullptr,
                    size_t m = 0) {
    const std::vector<double> tols = integ_tols_packed(opt, d_abs ? n : 0);
    return copy({{rows, d_rows, nrows, label}, {tf, d_tf, m, "tf"}, {d_abs ? tols.data() : nullptr, d_abs, tols.size(), "tolerances"}},
                hipMemcpyHostToDevice);
  }
  static int download(const std::vector<Row>& rows) { return copy(rows, hipMemcpyDeviceToHost); }
};

// tsnd | errors | dist | error_max | dist_max of an estimator (Args: MeshArgs, IntegArgs): their slots, and their way back
template <class Args>
void estimate_take(IntegCall& c, Args& a, int n) {
  const size_t nd = size_t(a.nb) + 1;
  c.d.take(&a.tsnd, nd), c.d.take(&a.errors, nd * n), c.d.take(&a.dist, nd * n), c.d.take(&a.error_max, nd), c.d.take(&a.dist_max, nd);
}
template <class Args>
std::vector<IntegCall::Row> estimate_rows(const Args& a, int n, double* tsnd, double* mesh_errors, double* mesh_dist, double* error_max,
                                          double* dist_max) {
  const size_t nd = size_t(a.nb) + 1;
  return {{tsnd, a.tsnd, nd, "results"}, {mesh_errors, a.errors, nd * n, "results"}, {mesh_dist, a.dist, nd * n, "results"},
          {error_max, a.error_max, nd, "error_max"}, {dist_max, a.dist_max, nd, "dist_max"}};
}

// the one entry of an ODE that holds its propagation kernels (registry.h: prop_home)
const asset_hip::KernelEntry* prop_entry(const char* ode) {
  const asset_hip::KernelEntry* ke = find_entry(ode, asset_hip::PROP_HOME_MODE, 0);
  return (ke && asset_hip::prop_home(ke->mode, ke->blocked != 0) && ke->table->meta[asset_hip::MF_KIND] == 1 && asset_hip::entry_has_prop(ke)) ? ke : nullptr;
}

// an ODE with event functions: a run-time module of kind 4 (asset_hip_jit_plugin), registered under its own name
const asset_hip::KernelEntry* event_entry(const char* module) {
  const asset_hip::KernelEntry* ke = find_entry(module, ASSET_HIP_FUNCTION, 0);
  return (ke && ke->table->meta[asset_hip::MF_KIND] == 4 && ke->table->k[asset_hip::K_PROP_EVENT]) ? ke : nullptr;
}

// ... propagated with its state-transition matrix: a run-time module of kind 6
const asset_hip::KernelEntry* event_stm_entry(const char* module) {
  const asset_hip::KernelEntry* ke = find_entry(module, ASSET_HIP_FUNCTION, 0);
  const bool ok = ke && ke->table->meta[asset_hip::MF_KIND] == 6 && ke->table->k[asset_hip::K_PROP_EVENT_STM] &&
                  ke->table->k[asset_hip::K_PROP_EVENT_JAC];
  return ok ? ke : nullptr;
}

// an ODE with its control law: a run-time module of kind 5 (asset_hip_jit_plugin), registered under its own name
const asset_hip::KernelEntry* ctrl_entry(const char* module) {
  const asset_hip::KernelEntry* ke = find_entry(module, ASSET_HIP_FUNCTION, 0);
  const bool ok = ke && ke->table->meta[asset_hip::MF_KIND] == 5 && ke->table->k[asset_hip::K_PROP_CTRL_BATCH] &&
                  ke->table->k[asset_hip::K_PROP_CTRL_STM] && ke->table->k[asset_hip::K_PROP_CTRL_JAC];
  return ok ? ke : nullptr;
}

// The checks every propagation shares, in their order -- the first that fails wins, all of them before the device is touched.  The
// caller has checked its pointers; `own` stands where its entry lookup and whatever only it checks come in that order, and gives the
// launch plan of the entry it found.
template <class Own>
int prop_checked(long long m, int ns, const asset_hip_integ_options* opt, const double* tf, int device, asset_hip::IntegOptions& o,
                 asset_hip::PropPlan& plan, Own own) {
  if (m < 1) return fail(ASSET_HIP_EINVAL, "m must be at least 1");
  if (ns < 1) return fail(ASSET_HIP_EINVAL, "ns must be at least 1");
  if (const int rc = own(plan)) return rc;
  if (const int rc = integ_options_checked(opt, o)) return rc;
  for (long long i = 0; i < m; i++)
    if (!std::isfinite(tf[i])) return fail(ASSET_HIP_EINVAL, "tf is not finite (problem " + std::to_string(i) + ")");
  if (plan.grid < 1 || plan.grid > 0x7fffffffLL || size_t(plan.lds_bytes) > 64 * 1024)
    return fail(ASSET_HIP_EINVAL, "the batch does not fit one launch (workgroups or LDS)");
  return use_device(device, "no HIP device visible: the propagation has no CPU fallback");
}

// y0 | tf | abs | rel at the head of the doubles and steps | status at the head of the ints (Args: PropArgs, PropCtrlArgs, PropEventArgs,
// PropEventStmArgs)
template <class Args>
void problems_take(IntegCall& c, Args& a, size_t m, int N, int n) {
  c.d.take(&a.y0, m * N), c.d.take(&a.tf, m), c.d.take(&a.abs_tols, n), c.d.take(&a.rel_tols, n);
  c.i.take(&a.steps, m * 2), c.i.take(&a.status, m);
}

// asset_hip_propagate* (Args = PropArgs: `name` an ODE, no `us`) and asset_hip_propagate_ctrl* (PropCtrlArgs: a module of kind 5)
template <class Args>
int propagate_impl(const char* name, const double* y0, long long m, const double* tf, int ns, const asset_hip_integ_options* opt, bool stm,
                   double* xs, double* us, double* jac, int* steps, int* status, double* xf_last, int device) {
  constexpr bool ctrl = std::is_same<Args, asset_hip::PropCtrlArgs>::value;
  if (!name || !y0 || !tf || !xs || (ctrl && !us) || (stm && !jac)) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = nullptr;
  Args a{};
  asset_hip::PropPlan plan;
  const int bad = prop_checked(m, ns, opt, tf, device, a.opt, plan, [&](asset_hip::PropPlan& p) {
    ke = ctrl ? ctrl_entry(name) : prop_entry(name);
    if (!ke && !ctrl)
      return fail(ASSET_HIP_ENOODE, std::string("no propagation kernels compiled for ode='") + name + "' (its LGL3 entry holds them)");
    if (!ke && (find_entry(name, ASSET_HIP_FUNCTION, 0) || prop_entry(name)))
      return fail(ASSET_HIP_ENOODE, std::string("'") + name + "' is not a controller module (asset_hip_jit_plugin, kind 5)");
    if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no controller module registered as '") + name + "' (asset_hip_jit_plugin, kind 5)");
    // (a controlled problem carries no control columns: the STM's plan is that of (n, 0, pv))
    p = asset_hip::propagate_plan(ke->xv, ctrl && stm ? 0 : ke->uv, ke->pv, m, stm ? 1 : 0);
    return 0;
  });
  if (bad) return bad;
  const int n = ke->xv, uv = ke->uv, N = n + 1 + uv + ke->pv, C = ctrl ? n + ke->pv : N - 1;
  // one allocation of doubles: y0 | tf | abs | rel | xs | (controller: us) | (stm: S | jac | xlast); one of ints: steps | status
  const size_t um = size_t(m), nsu = stm ? 1 : size_t(ns), sz_x = um * nsu * n, sz_u = ctrl ? um * nsu * uv : 0, sz_l = um * n;
  a.m = m, a.ns = int(nsu);
  a.group = plan.group, a.lanes = plan.lanes, a.passes = plan.passes;
  double* d_us = nullptr;
  IntegCall c;
  problems_take(c, a, um, N, n);
  c.d.take(&a.xs, sz_x), c.d.take(ctrl ? &d_us : nullptr, sz_u);
  if (stm) c.d.take(&a.S, sz_l * C), c.d.take(&a.jac, sz_l * (N + 1)), c.d.take(&a.xlast, sz_l);
  if (const int rc = c.allocate()) return rc;
  if (const int rc = c.upload(a.y0, y0, um * N, "y0", a.abs_tols, opt, n, a.tf, tf, um)) return rc;
  if constexpr (ctrl) a.us = d_us;
  void* kargs[] = {&a};
  const asset_hip::KernelTable& t = *ke->table;
  const int k_batch = ctrl ? asset_hip::K_PROP_CTRL_BATCH : asset_hip::K_PROP_BATCH, k_stm = ctrl ? asset_hip::K_PROP_CTRL_STM : asset_hip::K_PROP_STM,
            k_jac = ctrl ? asset_hip::K_PROP_CTRL_JAC : asset_hip::K_PROP_JAC;
  HIP_TRY_AS(asset_hip::klaunch(t.k[stm ? k_stm : k_batch], dim3(unsigned(plan.grid)), dim3(64), size_t(plan.lds_bytes), nullptr, kargs),
             ctrl ? "controller propagation kernel" : "propagation kernel");
  if (stm)
    HIP_TRY_AS(asset_hip::klaunch(t.k[k_jac], dim3(unsigned((m + 63) / 64)), dim3(64), 0, nullptr, kargs),
               ctrl ? "controller STM assembly kernel" : "STM assembly kernel");
  HIP_TRY_AS(hipDeviceSynchronize(), ctrl ? "controller propagation kernels" : "propagation kernels");
  return c.download({{xs, a.xs, sz_x, "states"}, {us, d_us, sz_u, "controls"}, {jac, a.jac, sz_l * (N + 1), "jac"},
                     {xf_last, a.xlast, sz_l, "xf_last"}, {steps, a.steps, um * 2, "steps"}, {status, a.status, um, "status"}});
}
// the launch plan of a propagation with events: a lane per problem, or with the STM the plan of prop_stm_kernel unchanged
asset_hip::PropPlan event_plan(const asset_hip::KernelEntry* ke, long long m, bool stm) {
  return asset_hip::propagate_plan(ke->xv, ke->uv, ke->pv, m, stm ? 1 : 0);
}

// asset_hip_propagate_events (Args = PropEventArgs: a module of kind 4, no `jac` / `ev_jac`) and asset_hip_propagate_events_stm
// (PropEventStmArgs: a module of kind 6; `ev_jac` may be null, then ev_S is neither allocated nor written)
template <class Args>
int propagate_events_impl(const char* module, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt, int ne,
                          const int* direction, const int* stop, double event_tol, int max_event_iters, int max_locs, double* xf, double* jac,
                          double* t_end, int* stopped, int* ev_count, double* ev_rows, double* ev_resid, int* ev_conv, double* ev_jac,
                          int* steps, int* status, int device) {
  constexpr bool stm = std::is_same<Args, asset_hip::PropEventStmArgs>::value;
  if (!module || !y0 || !tf || !direction || !stop || !xf || (stm && !jac) || !t_end || !stopped || !ev_count || !ev_rows || !ev_resid ||
      !ev_conv)
    return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = nullptr;
  Args a{};
  asset_hip::PropPlan plan;
  const int bad = prop_checked(m, 1, opt, tf, device, a.opt, plan, [&](asset_hip::PropPlan& p) {
    ke = stm ? event_stm_entry(module) : event_entry(module);
    if (!ke && (stm ? event_entry(module) : event_stm_entry(module)))
      return fail(ASSET_HIP_ENOODE, std::string("'") + module + "' is an event module of kind " + (stm ? "4" : "6") + ": this call takes one of kind " +
                                        (stm ? "6 (asset_hip_propagate_events takes it)" : "4 (asset_hip_propagate_events_stm takes it)"));
    if (!ke)
      return fail(ASSET_HIP_ENOODE, std::string("no event module registered as '") + module + "' (asset_hip_jit_plugin, kind " + (stm ? "6)" : "4)"));
    if (ne != ke->orr) return fail(ASSET_HIP_EINVAL, "ne is " + std::to_string(ne) + " but the module has " + std::to_string(ke->orr) + " events");
    if (!(event_tol > 0.0)) return fail(ASSET_HIP_EINVAL, "event_tol must be positive");
    if (max_event_iters < 1) return fail(ASSET_HIP_EINVAL, "max_event_iters must be at least 1");
    if (max_locs < 1) return fail(ASSET_HIP_EINVAL, "max_locs must be at least 1");
    for (int j = 0; j < ne; j++) {
      if (direction[j] < -1 || direction[j] > 1) return fail(ASSET_HIP_EINVAL, "direction must be -1, 0 or 1 (event " + std::to_string(j) + ")");
      if (stop[j] < 0) return fail(ASSET_HIP_EINVAL, "stop must not be negative (event " + std::to_string(j) + ")");
      if (stop[j] > max_locs)
        return fail(ASSET_HIP_EINVAL, "stop exceeds max_locs: the stopping occurrence would not be located (event " + std::to_string(j) + ")");
    }
    p = event_plan(ke, m, stm);
    return 0;
  });
  if (bad) return bad;
  const int n = ke->xv, N = ke->xv + 1 + ke->uv + ke->pv, C = N - 1;
  // one allocation of doubles: y0 | tf | abs | rel | xf | t_end | ev_rows | ev_resid | (stm: S | jac | (ev_jac wanted: ev_S | ev_jac));
  // one of ints: steps | status | stopped | ev_count | ev_conv
  const size_t um = size_t(m), sz_x = um * n, sz_e = um * ne * size_t(max_locs), sz_r = sz_e * (n + 1), sz_c = um * ne;
  const size_t sz_j = stm ? sz_x * (N + 1) : 0, sz_ej = stm && ev_jac ? sz_e * n * (N + 1) : 0;
  a.m = m, a.lanes = plan.lanes, a.max_iters = max_event_iters, a.max_locs = max_locs, a.event_tol = event_tol;
  for (int j = 0; j < asset_hip::PROP_EVENT_MAX; j++) a.direction[j] = j < ne ? direction[j] : 0, a.stop[j] = j < ne ? stop[j] : 0;
  double* d_jac = nullptr;
  double* d_ev_jac = nullptr;
  IntegCall c;
  problems_take(c, a, um, N, n);
  c.d.take(&a.xf, sz_x), c.d.take(&a.t_end, um), c.d.take(&a.ev_rows, sz_r), c.d.take(&a.ev_resid, sz_e);
  if constexpr (stm) {
    a.group = plan.group, a.passes = plan.passes;
    c.d.take(&a.S, sz_x * C), c.d.take(&a.jac, sz_j);
    c.d.take(ev_jac ? &a.ev_S : nullptr, ev_jac ? sz_e * n * C : 0), c.d.take(ev_jac ? &a.ev_jac : nullptr, sz_ej);
  }
  c.i.take(&a.stopped, um), c.i.take(&a.ev_count, sz_c), c.i.take(&a.ev_conv, sz_e);
  if (const int rc = c.allocate()) return rc;
  if (const int rc = c.upload(a.y0, y0, um * N, "y0", a.abs_tols, opt, n, a.tf, tf, um)) return rc;
  if constexpr (stm) d_jac = a.jac, d_ev_jac = a.ev_jac;
  void* kargs[] = {&a};
  HIP_TRY_AS(asset_hip::klaunch(ke->table->k[stm ? asset_hip::K_PROP_EVENT_STM : asset_hip::K_PROP_EVENT], dim3(unsigned(plan.grid)), dim3(64),
                                size_t(plan.lds_bytes), nullptr, kargs), "event propagation kernel");
  if (stm) {
    const size_t items = um * (ev_jac ? 1 + size_t(ne) * size_t(max_locs) : 1);
    if ((items + 63) / 64 > 0x7fffffffULL) return fail(ASSET_HIP_EINVAL, "the batch does not fit one launch (workgroups or LDS)");
    HIP_TRY_AS(asset_hip::klaunch(ke->table->k[asset_hip::K_PROP_EVENT_JAC], dim3(unsigned((items + 63) / 64)), dim3(64), 0, nullptr, kargs),
               "event STM assembly kernel");
  }
  HIP_TRY_AS(hipDeviceSynchronize(), "event propagation kernel");
  return c.download({{xf, a.xf, sz_x, "states"}, {jac, d_jac, sz_j, "jac"}, {t_end, a.t_end, um, "t_end"}, {ev_rows, a.ev_rows, sz_r, "ev_rows"},
                     {ev_resid, a.ev_resid, sz_e, "ev_resid"}, {ev_jac, d_ev_jac, sz_ej, "ev_jac"}, {stopped, a.stopped, um, "stopped"},
                     {ev_count, a.ev_count, sz_c, "ev_count"}, {ev_conv, a.ev_conv, sz_e, "ev_conv"}, {steps, a.steps, um * 2, "steps"},
                     {status, a.status, um, "status"}});
}
}  // namespace

extern "C" {

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
  if (const int rc = use_device(device, "no HIP device visible: the estimator has no CPU fallback")) return rc;
  // one allocation: traj | yvec | hs | tsnd | errors | dist | error_max | dist_max
  const size_t sz_traj = size_t(nnodes) * N;
  asset_hip::MeshArgs a{};
  a.nb = nb;
  IntegCall c;
  c.d.take(&a.traj, sz_traj), c.d.take(&a.yvec, size_t(nb) * n), c.d.take(&a.hs, nb);
  estimate_take(c, a, n);
  if (const int rc = c.allocate()) return rc;
  if (const int rc = c.upload(a.traj, traj, sz_traj, "traj")) return rc;
  HIP_TRY_AS(asset_hip::entry_mesh(ke, a, nullptr), "mesh kernels");
  return c.download(estimate_rows(a, n, tsnd, mesh_errors, mesh_dist, error_max, dist_max));
}

// The integrator-based estimate (integ_kernels.h).  Every input is checked before the device is touched.
int asset_hip_mesh_error_integrator(const char* ode, int mode, int blocked, const double* traj, int nnodes,
                                    const asset_hip_integ_options* opt, double* tsnd, double* mesh_errors, double* mesh_dist,
                                    double* error_max, double* dist_max, double* xend, int* steps, int* status, int device) {
  if (!ode || !traj || !tsnd || !mesh_errors || !mesh_dist) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = find_entry(ode, mode, blocked);
  if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no device code compiled for ode='") + ode + "' in this mode");
  if (ke->table->meta[asset_hip::MF_KIND] != 1 || !asset_hip::entry_has_integ(ke))
    return fail(ASSET_HIP_EINVAL, "this entry is not a transcription of an ODE");
  const int K = asset_hip::interp_basis(mode).cs - 1, n = ke->xv, N = ke->xv + 1 + ke->uv + ke->pv;
  if (nnodes < 2 || (nnodes - 1) % K != 0)
    return fail(ASSET_HIP_EINVAL, "the trajectory must hold nb*(cs-1)+1 nodes with nb >= 1 blocks");
  if (const int rc = traj_times_checked(traj, nnodes, N, n)) return rc;
  asset_hip::IntegArgs a{};
  a.nb = (nnodes - 1) / K;
  if (const int rc = integ_options_checked(opt, a.opt)) return rc;
  if (const int rc = use_device(device, "no HIP device visible: the estimator has no CPU fallback")) return rc;
  // one allocation of doubles: traj | abs | rel | xend | e | tsnd | errors | dist | error_max | dist_max | max_err; one of ints: steps | status
  const size_t sz_traj = size_t(nnodes) * N, nint = size_t(nnodes) - 1;
  double* d_max_err = nullptr;
  IntegCall c;
  c.d.take(&a.traj, sz_traj), c.d.take(&a.abs_tols, n), c.d.take(&a.rel_tols, n), c.d.take(&a.xend, nint * n), c.d.take(&a.e, nint * n);
  estimate_take(c, a, n);
  c.d.take(&d_max_err, 1);
  c.i.take(&a.steps, nint * 2), c.i.take(&a.status, nint);
  if (const int rc = c.allocate()) return rc;
  a.max_err = reinterpret_cast<unsigned long long*>(d_max_err);
  if (const int rc = c.upload(a.traj, traj, sz_traj, "traj", a.abs_tols, opt, n)) return rc;
  HIP_TRY_AS(asset_hip::entry_integ(ke, a, nullptr), "integrator mesh-error kernels");
  HIP_TRY_AS(hipDeviceSynchronize(), "integrator mesh-error kernels");
  std::vector<IntegCall::Row> rows = estimate_rows(a, n, tsnd, mesh_errors, mesh_dist, error_max, dist_max);
  rows.insert(rows.end(), {{xend, a.xend, nint * n, "xend"}, {steps, a.steps, nint * 2, "steps"}, {status, a.status, nint, "status"}});
  return c.download(rows);
}

// ---------------------------------------------------------------------------------------------- batched propagation

int asset_hip_propagate(const char* ode, const double* y0, long long m, const double* tf, int ns, const asset_hip_integ_options* opt,
                        double* xs, int* steps, int* status, int device) {
  return propagate_impl<asset_hip::PropArgs>(ode, y0, m, tf, ns, opt, false, xs, nullptr, nullptr, steps, status, nullptr, device);
}
int asset_hip_propagate_stm(const char* ode, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt,
                            double* xf, double* jac, int* steps, int* status, int device) {
  return propagate_impl<asset_hip::PropArgs>(ode, y0, m, tf, 1, opt, true, xf, nullptr, jac, steps, status, nullptr, device);
}
int asset_hip_propagate_stm_lanes(const char* ode, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt,
                                  double* xf, double* jac, int* steps, int* status, double* xf_last, int device) {
  if (!xf_last) return fail(ASSET_HIP_EINVAL, "null argument");
  return propagate_impl<asset_hip::PropArgs>(ode, y0, m, tf, 1, opt, true, xf, nullptr, jac, steps, status, xf_last, device);
}
int asset_hip_event_module_sizes(const char* module, int* xv, int* uv, int* pv, int* ne) {
  if (!module) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = event_entry(module);
  if (!ke) ke = event_stm_entry(module);             // (a module of kind 4 or of kind 6: the same fields)
  if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no event module registered as '") + module + "'");
  if (xv) *xv = ke->xv;
  if (uv) *uv = ke->uv;
  if (pv) *pv = ke->pv;
  if (ne) *ne = ke->orr;
  return 0;
}

int asset_hip_propagate_events(const char* module, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt,
                               int ne, const int* direction, const int* stop, double event_tol, int max_event_iters, int max_locs,
                               double* xf, double* t_end, int* stopped, int* ev_count, double* ev_rows, double* ev_resid, int* ev_conv,
                               int* steps, int* status, int device) {
  return propagate_events_impl<asset_hip::PropEventArgs>(module, y0, m, tf, opt, ne, direction, stop, event_tol, max_event_iters, max_locs, xf,
                                                         nullptr, t_end, stopped, ev_count, ev_rows, ev_resid, ev_conv, nullptr, steps, status,
                                                         device);
}
int asset_hip_propagate_events_stm_plan(const char* module, long long m, long long* out) {
  if (!module || !out) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = event_stm_entry(module);
  if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no event module of kind 6 registered as '") + module + "'");
  const asset_hip::PropPlan p = event_plan(ke, m, true);
  if (p.grid < 1) return fail(ASSET_HIP_EINVAL, "m must be at least 1");
  const long long v[7] = {p.group, p.lanes, p.passes, p.problems_per_wg, p.lds_bytes, p.grid, p.columns};
  for (int k = 0; k < 7; k++) out[k] = v[k];
  return 0;
}
int asset_hip_propagate_events_stm(const char* module, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt,
                                   int ne, const int* direction, const int* stop, double event_tol, int max_event_iters, int max_locs,
                                   double* xf, double* jac, double* t_end, int* stopped, int* ev_count, double* ev_rows, double* ev_resid,
                                   int* ev_conv, double* ev_jac, int* steps, int* status, int device) {
  return propagate_events_impl<asset_hip::PropEventStmArgs>(module, y0, m, tf, opt, ne, direction, stop, event_tol, max_event_iters, max_locs,
                                                            xf, jac, t_end, stopped, ev_count, ev_rows, ev_resid, ev_conv, ev_jac, steps,
                                                            status, device);
}

// ---- propagation with a controller (propagate_ctrl_kernels.h): propagate_impl against a module of kind 5
int asset_hip_propagate_ctrl(const char* module, const double* y0, long long m, const double* tf, int ns, const asset_hip_integ_options* opt,
                             double* xs, double* us, int* steps, int* status, int device) {
  return propagate_impl<asset_hip::PropCtrlArgs>(module, y0, m, tf, ns, opt, false, xs, us, nullptr, steps, status, nullptr, device);
}
int asset_hip_propagate_ctrl_stm(const char* module, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt,
                                 double* xf, double* uf, double* jac, int* steps, int* status, int device) {
  return propagate_impl<asset_hip::PropCtrlArgs>(module, y0, m, tf, 1, opt, true, xf, uf, jac, steps, status, nullptr, device);
}
int asset_hip_propagate_ctrl_stm_lanes(const char* module, const double* y0, long long m, const double* tf, const asset_hip_integ_options* opt,
                                       double* xf, double* uf, double* jac, int* steps, int* status, double* xf_last, int device) {
  if (!xf_last) return fail(ASSET_HIP_EINVAL, "null argument");
  return propagate_impl<asset_hip::PropCtrlArgs>(module, y0, m, tf, 1, opt, true, xf, uf, jac, steps, status, xf_last, device);
}
int asset_hip_controller_module_sizes(const char* module, int* xv, int* uv, int* pv) {
  if (!module) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::KernelEntry* ke = ctrl_entry(module);
  if (!ke) return fail(ASSET_HIP_ENOODE, std::string("no controller module registered as '") + module + "'");
  if (xv) *xv = ke->xv;
  if (uv) *uv = ke->uv;
  if (pv) *pv = ke->pv;
  return 0;
}

int asset_hip_propagate_plan(int xv, int uv, int pv, long long m, int stm, long long* out) {
  if (!out) return fail(ASSET_HIP_EINVAL, "null argument");
  const asset_hip::PropPlan p = asset_hip::propagate_plan(xv, uv, pv, m, stm);
  if (p.grid < 1) return fail(ASSET_HIP_EINVAL, "sizes must satisfy xv >= 1, uv >= 0, pv >= 0, m >= 1");
  const long long v[7] = {p.group, p.lanes, p.passes, p.problems_per_wg, p.lds_bytes, p.grid, p.columns};
  for (int k = 0; k < 7; k++) out[k] = v[k];
  return 0;
}

int asset_hip_rk_table(const char* which, double* out, int n) {
  if (!which || !out) return fail(ASSET_HIP_EINVAL, "bad rk table query");
  const asset_hip::RkTab& t = asset_hip::h_rk_tab;
  const double* src = nullptr;
  int cnt = 0;
  if (!std::strcmp(which, "a")) src = &t.a[0][0], cnt = 144;
  else if (!std::strcmp(which, "c")) src = t.c, cnt = 12;
  else if (!std::strcmp(which, "b")) src = t.b, cnt = 13;
  else if (!std::strcmp(which, "bhat")) src = t.bhat, cnt = 13;
  else return fail(ASSET_HIP_EINVAL, "unknown table name");
  if (n < cnt) return fail(ASSET_HIP_EINVAL, "output buffer too small");
  for (int i = 0; i < cnt; i++) out[i] = src[i];
  return cnt;
}

// ---------------------------------------------------------------------------------------------- trajectory table

struct asset_hip_traj_table {
  const asset_hip::KernelEntry* ke = nullptr;
  int nb = 0, nnodes = 0, N = 0, n = 0, device = 0, cus = 256;
  double t0 = 0.0, tf = 0.0;
  asset_hip::Stream stream;                 // (first: it goes after the buffers)
  DeviceBuffer<double> buf;                 // traj | xdot | tb, resident
  asset_hip::InterpArgs a{};
  // staging of the host-pointer entry point (grown on demand): times | out | dout for as many queries as fit, and the counter
  DeviceBuffer<double> stage;
  DeviceBuffer<unsigned long long> count;
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
  if (const int rc = traj_times_checked(traj, nnodes, N, n)) return rc;
  if (const int rc = use_device(device, "no HIP device visible: the trajectory table has no CPU fallback")) return rc;
  std::unique_ptr<asset_hip_traj_table> t(new (std::nothrow) asset_hip_traj_table());
  if (!t) return fail(ASSET_HIP_EINVAL, "out of host memory");
  t->ke = ke, t->nb = nb, t->nnodes = nnodes, t->N = N, t->n = n, t->device = device;
  t->t0 = traj[n], t->tf = traj[size_t(nnodes - 1) * N + n];
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) t->cus = prop.multiProcessorCount;
  const size_t sz_traj = size_t(nnodes) * N, sz_xd = size_t(nnodes) * n, total = sz_traj + sz_xd + size_t(nb) + 1;
  HIP_TRY_AS(t->stream.create(), "hipStreamCreate");
  HIP_TRY_AS(t->buf.allocate(total), "hipMalloc(table)");
  HIP_TRY_AS(t->count.allocate(1), "hipMalloc(counter)");
  t->a.nb = nb, t->a.nq = 0;
  t->a.traj = t->buf.get(), t->a.xdot = t->buf.get() + sz_traj, t->a.tb = t->buf.get() + sz_traj + sz_xd;
  HIP_TRY_AS(hipMemcpyAsync(t->buf.get(), traj, sz_traj * sizeof(double), hipMemcpyHostToDevice, t->stream.get()), "hipMemcpy(traj)");
  HIP_TRY_AS(asset_hip::entry_interp_table(ke, t->a, t->stream.get()), "interp_xdot_kernel");
  HIP_TRY_AS(hipStreamSynchronize(t->stream.get()), "trajectory table set-up");
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
  return traj_table_launch(t, d_times, n, deriv, d_out, d_dout, d_n_outside, stream_or(t, stream));
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
  hipStream_t st = t->stream.get();
  if (size_t(n) * (1 + 2 * N) > t->stage.size()) {   // times | out | dout
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(t->stage.allocate(size_t(n) * (1 + 2 * N)));
  }
  const size_t cap_q = t->stage.size() / (1 + 2 * N);
  double *d_times = t->stage.get(), *d_out = d_times + cap_q, *d_dout = d_out + cap_q * N;
  HIP_TRY(hipMemcpyAsync(d_times, times, size_t(n) * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(t->count.get(), 0, sizeof(unsigned long long), st));
  const int rc = traj_table_launch(t, d_times, n, deriv, d_out, d_dout, t->count.get(), st);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, size_t(n) * N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (deriv) HIP_TRY(hipMemcpyAsync(dout, d_dout, size_t(n) * N * sizeof(double), hipMemcpyDeviceToHost, st));
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, t->count.get(), sizeof cnt, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
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
  if (t->stream.get()) (void)hipStreamSynchronize(t->stream.get());
  (void)hipDeviceSynchronize();          // (queries enqueued on the caller's streams still read the table)
  delete t;
}

// ---------------------------------------------------------------------------------------------- on-device assembly

int asset_hip_kkt_map_query(int ir, int orr, int plain_function, int nseg, const int32_t* slot_locations, long long nvalues,
                            int accumulate, long long* map_len, int32_t* map_words, int* nmulti, int32_t* multi_ptr,
                            int32_t* multi_loc, long long* lo, long long* hi) {
  if (ir <= 0 || orr <= 0 || nseg <= 0 || !slot_locations || nvalues <= 0) return fail(ASSET_HIP_EINVAL, "bad kkt map arguments");
  asset_hip::KktMap m;
  const char* err = nullptr;
  if (const int rc = asset_hip::build_kkt_map(ir, orr, plain_function != 0, nseg, slot_locations, nvalues, accumulate, m, &err))
    return fail(rc, err);
  if (map_len) *map_len = (long long)m.words.size();
  if (nmulti) *nmulti = int(m.multi_loc.size());
  if (lo) *lo = m.lo;
  if (hi) *hi = m.hi;
  if (map_words) std::copy(m.words.begin(), m.words.end(), map_words);
  if (multi_ptr) std::copy(m.multi_ptr.begin(), m.multi_ptr.end(), multi_ptr);
  if (multi_loc) std::copy(m.multi_loc.begin(), m.multi_loc.end(), multi_loc);
  return 0;
}

int asset_hip_defect_set_kkt_map(asset_hip_defect_t h, const int32_t* slot_locations, long long nvalues, int accumulate) {
  if (!h || !slot_locations || nvalues <= 0) return fail(ASSET_HIP_EINVAL, "bad kkt map arguments");
  HIP_TRY(hipSetDevice(h->device));
  // FAILURE-ATOMIC: the old map is dropped first (two maps side by side would not fit at the sizes that matter), the new one is built
  // and uploaded through locals and committed by the last statement.  A failed call leaves a handle with no map -- the assembled
  // kinds refuse -- never part of one.
  h->kmap = {};
  asset_hip::KktMap m;
  const char* err = nullptr;
  if (const int rc = asset_hip::build_kkt_map(h->ke->ir, h->ke->orr, h->ke->mode == ASSET_HIP_FUNCTION, h->nseg, slot_locations, nvalues,
                                              accumulate, m, &err))
    return fail(rc, err);
  asset_hip_defect::DeviceKktMap g;
  g.value_lo = m.lo, g.value_hi = m.hi, g.nvalues = nvalues;
  HIP_TRY_AS(upload(g.map, m.words), "uploading the kkt map");
  if (!m.multi_loc.empty()) {   // staging cells and the reduction lists
    HIP_TRY_AS(g.stage.allocate(size_t(m.multi_ptr.back())), "hipMalloc(kkt staging cells)");
    HIP_TRY_AS(hipMemset(g.stage.get(), 0, g.stage.size() * sizeof(double)), "hipMemset(kkt staging cells)");
    HIP_TRY_AS(upload(g.multi_ptr, m.multi_ptr), "uploading the kkt reduction lists");
    HIP_TRY_AS(upload(g.multi_loc, m.multi_loc), "uploading the kkt reduction lists");
  }
  h->kmap = std::move(g);
  return 0;
}

int asset_hip_defect_eval_assembled_device(asset_hip_defect_t h, int what, const double* dX, const double* dL,
                                           double* d_fx_blocks, double* d_agx_blocks, double* d_kkt_values,
                                           void* stream) {
  what &= 0xff;   // (no blocks are written: ASSET_HIP_KEEP_HESSIAN_SLOTS has nothing to act on)
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (what < ASSET_HIP_JAC) return fail(ASSET_HIP_EINVAL, "assembled evaluation needs a kind that produces KKT entries");
  if (!h->kmap.map) return fail(ASSET_HIP_EINVAL, "no kkt map: call asset_hip_defect_set_kkt_map first");
  if (!d_kkt_values) return fail(ASSET_HIP_EINVAL, "kkt value array is null");
  HIP_TRY(hipSetDevice(h->device));
  // the dense stage places its accumulators in the value array itself (defect_kernels.h, ASM instantiations)
  return launch(h, what, dX, dL, d_fx_blocks, d_agx_blocks, nullptr, stream_or(h, stream), d_kkt_values);
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

// the gather tables of a handle's index tables and the block buffers they read
static hipError_t build_rhs_tables(const asset_hip_defect* h, asset_hip_defect::RhsTables& r) {
  std::vector<int> rows, ptr, src;
  hipError_t e;
  r.fx_long_from = build_rhs_csr(h->mesh.h_cindex, rows, ptr, src);
  r.n_fx_rows = int(rows.size());
  if ((e = upload(r.fx_rows, rows, 1)) != hipSuccess || (e = upload(r.fx_ptr, ptr, 1)) != hipSuccess || (e = upload(r.fx_src, src, 1)) != hipSuccess) return e;
  r.gx_long_from = build_rhs_csr(h->mesh.h_vindex, rows, ptr, src);
  r.n_gx_rows = int(rows.size());
  if ((e = upload(r.gx_rows, rows, 1)) != hipSuccess || (e = upload(r.gx_ptr, ptr, 1)) != hipSuccess || (e = upload(r.gx_src, src, 1)) != hipSuccess) return e;
  if ((e = r.fxb.allocate(size_t(h->nseg) * h->ke->orr)) != hipSuccess) return e;
  return r.agxb.allocate(size_t(h->nseg) * h->ke->ir);
}

int asset_hip_defect_eval_kkt_device(asset_hip_defect_t h, int what, const double* dX, const double* dL, double* d_FXE,
                                     double* d_AGX, double* d_kkt_values, void* stream) {
  what &= 0xff;   // (no blocks are written: ASSET_HIP_KEEP_HESSIAN_SLOTS has nothing to act on)
  if (!h) return fail(ASSET_HIP_EINVAL, "null handle");
  if (!d_FXE) return fail(ASSET_HIP_EINVAL, "FXE is null");
  const bool want_kkt = wants_kkt(what), want_agx = wants_multipliers(what);
  if (want_kkt && (!h->kmap.map || !d_kkt_values)) return fail(ASSET_HIP_EINVAL, "no kkt map / value array for a kind that fills the matrix");
  if (want_agx && !d_AGX) return fail(ASSET_HIP_EINVAL, "AGX is null for a kind that produces the adjoint gradient");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = stream_or(h, stream);
  if (!h->rhs.agxb) {   // the gather tables, once per mesh: built into a local, committed only when all of them exist
    asset_hip_defect::RhsTables fresh;
    HIP_TRY_AS(build_rhs_tables(h, fresh), "building the RHS gather tables");
    h->rhs = std::move(fresh);
  }
  const asset_hip_defect::RhsTables& r = h->rhs;
  int rc = launch(h, what, dX, dL, r.fxb.get(), want_agx ? r.agxb.get() : nullptr, nullptr, st, want_kkt ? d_kkt_values : nullptr);
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
  HIP_TRY(gather(d_FXE, r.fxb.get(), r.fx_rows.get(), r.fx_ptr.get(), r.fx_src.get(), r.n_fx_rows, r.fx_long_from));
  if (want_agx) HIP_TRY(gather(d_AGX, r.agxb.get(), r.gx_rows.get(), r.gx_ptr.get(), r.gx_src.get(), r.n_gx_rows, r.gx_long_from));
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
  if (!h->kmap.map) return fail(ASSET_HIP_EINVAL, "no kkt map: call asset_hip_defect_set_kkt_map first");
  HIP_TRY(hipSetDevice(h->device));
  asset_hip_defect::DeviceKktMap& k = h->kmap;
  const size_t nfx = size_t(h->nseg) * h->ke->orr, nagx = size_t(h->nseg) * h->ke->ir;
  const size_t nval = size_t(k.value_hi - k.value_lo);
  if (!k.h_values) {   // (the pinned mirror is the second of the pair: a call that got only the first starts over)
    HIP_TRY(k.d_values.allocate(nval));
    HIP_TRY(k.h_values.allocate(nval));
  }
  int rc = stage_inputs(h, X, L, fx_blocks, agx_blocks, false);
  if (rc) return rc;
  const asset_hip_defect::HostStaging& s = h->staging;
  hipStream_t st = h->stream.get();
  HIP_TRY(hipMemsetAsync(k.d_values.get(), 0, sizeof(double) * nval, st));
  // The device array covers [value_lo, value_hi) of the caller's: bias the base address so that locations index it
  // directly (integer arithmetic: the biased address is only ever used with offsets >= value_lo).
  double* biased = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(k.d_values.get()) - uintptr_t(k.value_lo) * sizeof(double));
  rc = asset_hip_defect_eval_assembled_device(h, what, s.X.get(), L ? s.L.get() : nullptr, fx_blocks ? s.fx.get() : nullptr,
                                              agx_blocks ? s.agx.get() : nullptr, biased, st);
  if (rc) return rc;
  if (fx_blocks) HIP_TRY(hipMemcpyAsync(fx_blocks, s.fx.get(), sizeof(double) * nfx, hipMemcpyDeviceToHost, st));
  if (agx_blocks && what != ASSET_HIP_JAC) HIP_TRY(hipMemcpyAsync(agx_blocks, s.agx.get(), sizeof(double) * nagx, hipMemcpyDeviceToHost, st));
  if (target_zeroed) {
    // the caller's range holds zeros (it was just cleared and this constraint is the first to fill it): the values go
    // straight into it -- by DMA when the array is page-locked (asset_hip_host_register), through the driver's staging
    // otherwise -- and no host pass over the values is needed at all
    HIP_TRY(hipMemcpyAsync(kkt_values + k.value_lo, k.d_values.get(), sizeof(double) * nval, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
  }
  HIP_TRY(hipMemcpyAsync(k.h_values.get(), k.d_values.get(), sizeof(double) * nval, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // accumulate, as the reference's fill does: O(nnz) contiguous adds, split over a few threads (memory-bound)
  double* dst = kkt_values + k.value_lo;
  const double* src = k.h_values.get();
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

// The map of the on-device KKT assembly (asset_hip_defect_set_kkt_map), built on the host: which solver location every
// accumulator entry goes to and how -- plain store, atomic add, or a staged cell with an ordered reduction.  Pure host
// arithmetic: no HIP header, no device, no handle (asset_hip_kkt_map_query hands it out as it is).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../../include/asset_hip.h"

namespace asset_hip {

struct KktMap {
  std::vector<int32_t> words;                  // map word of every accumulator entry, fragment order (defect_kernels.h, ASM)
  std::vector<int32_t> multi_ptr, multi_loc;   // the staged locations and their cells (asm_reduce_kernel)
  long long lo = 0, hi = 0;                    // the range of the value array the map touches
};

// 0, or the error code with *err set.  IR / OR: rows of the function; plain_function: entries are placed slot by slot.
inline int build_kkt_map(int IR, int OR, bool plain_function, int nseg, const int32_t* slot_locations, long long nvalues,
                         int accumulate, KktMap& out, const char** err) {
  auto fail = [&](int code, const char* msg) { *err = msg; return code; };
  const int NK = IR * (IR + 1) / 2 + OR * IR;   // slots of a block, the reference's order (DenseFunctionBase.h:1070-1088)
  const size_t nslots = size_t(nseg) * NK;
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
  std::vector<unsigned char> is_h(NK, 0);
  for (int c = 0, k = 0; c < IR; c++) {
    for (int j = c; j < IR; j++) is_h[k++] = 1;
    k += OR;
  }
  auto staged = [&](size_t i) {
    const int32_t m = slot_locations[i];
    return m >= 0 && is_h[i % size_t(NK)] && uses[size_t(m - lo)] >= 3;
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
    for (size_t i = 0; i < nslots; i++)
      if (staged(i)) cnt[multi_of[slot_locations[i]]]++;
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
        else if (staged(i)) enc[i] = -(int32_t(nvalues) + fill[multi_of[m]]++ + 2);
        else if (multi_of.count(m))   // (asm_reduce_kernel ASSIGNS the staged sum: an add into the same location would be lost)
          return fail(ASSET_HIP_EINVAL, "a Jacobian slot names a location that is staged for three or more Hessian slots");
        else enc[i] = -(m + 2);
      }
    }
  }
  std::vector<int32_t> map;
  if (plain_function) {   // plain functions place their entries slot by slot (func_kernels.h)
    map = enc;
  } else {
    // fragment order of the LGL dense stage (defect_kernels.h, ASM): for every segment (4*tiles) rows of 64 lanes;
    // lane (lr = l & 15, lk = l >> 4), entry v of an accumulator tile is block column c = 16ct + lk + 4v and row
    // r = 16rt + lr (H, lower-triangle tiles first, tix = rt(rt+1)/2 + ct) or defect row jr = 16jt + lr
    // (J, tile ct*TJ + jt); -1 where that entry is no KKT slot.
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
    map.resize(size_t(nseg) * NF * 64);
    for (int V = 0; V < nseg; V++) {
      int32_t* dst = map.data() + size_t(V) * NF * 64;
      const int32_t* encV = enc.data() + size_t(V) * NK;
      for (size_t e = 0; e < size_t(NF) * 64; e++) dst[e] = slot_of[e] < 0 ? -1 : encV[slot_of[e]];
    }
  }
  out.words.swap(map), out.multi_ptr.swap(multi_ptr), out.multi_loc.swap(multi_loc), out.lo = lo, out.hi = hi;
  return 0;
}

}  // namespace asset_hip

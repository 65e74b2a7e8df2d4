"""csrc/capi/arena.h -- the sizes and places of the device arrays of the integrating entry points (capi.hip: IntegCall) -- compiled with
plain g++ into a program of its own, no device and no HIP header: offsets are the running sums in the order of taking, total() is the
sum, a count of 0 is legal, bind() puts every destination at base + offset and leaves an absent array's pointer alone, a sum that
leaves size_t is reported, and the layouts of the five entry points tile [0, total) exactly at small sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "capi/arena.h"
using asset_hip::Arena;

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// an arena that remembers what was taken from it: the slots must tile [0, total) in order
template <class T>
struct Layout {
  Arena<T> a;
  std::vector<size_t> off, cnt;
  void take(size_t count) { off.push_back(a.take(count)), cnt.push_back(count); }
  size_t tiled() const {
    size_t at = 0;
    for (size_t k = 0; k < off.size(); k++) {
      CHECK(off[k] == at);          // no gap, no overlap: a slot starts where the one before it ends
      at += cnt[k];
    }
    CHECK(at == a.total() && !a.overflowed());
    return at;
  }
};

int main() {
  {  // offsets are running sums; a count of 0 is legal; bind() resolves to base + offset and skips a null destination
    Arena<double> a;
    double *p = nullptr, *q = nullptr, *z = nullptr, *absent = nullptr;
    const double* r = nullptr;
    CHECK(a.total() == 0);
    CHECK(a.take(&p, 7) == 0 && a.total() == 7);
    CHECK(a.take(&z, 0) == 7 && a.total() == 7);
    CHECK(a.take(&r, 3) == 7 && a.total() == 10);
    CHECK(a.take(false ? &absent : nullptr, 0) == 10);
    CHECK(a.take(5) == 10 && a.total() == 15);
    CHECK(a.take(&q, 1) == 15 && a.total() == 16 && !a.overflowed());
    std::vector<double> mem(a.total());
    a.bind(mem.data());
    CHECK(p == mem.data() && z == mem.data() + 7 && r == mem.data() + 7 && q == mem.data() + 15 && absent == nullptr);
    Arena<int> none;                 // nothing taken: nothing to bind, also to a null base
    none.bind(nullptr);
    CHECK(none.total() == 0);
  }
  {  // a sum that leaves size_t is reported, and total() stays one that can be multiplied by sizeof(T)
    Arena<double> a;
    a.take(size_t(-1) / sizeof(double) - 1);
    CHECK(!a.overflowed());
    a.take(1);
    CHECK(!a.overflowed() && a.total() == size_t(-1) / sizeof(double));
    a.take(1);
    CHECK(a.overflowed() && a.total() == size_t(-1) / sizeof(double));
    Arena<int> b;
    b.take(size_t(-1));
    CHECK(b.overflowed() && b.total() == 0);
  }
  // the five layouts, by their size formulas (include/asset_hip.h: the array shapes)
  const size_t n = 5, N = 8, m = 3, ns = 4, uv = 2, pv = 0, ne = 2, locs = 3, cs = 4, nb = 3, nnodes = nb * (cs - 1) + 1, nint = nnodes - 1;
  {  // asset_hip_mesh_error_deboor: traj | yvec | hs | tsnd | errors | dist | error_max | dist_max
    Layout<double> d;
    for (size_t c : {nnodes * N, nb * n, nb, nb + 1, (nb + 1) * n, (nb + 1) * n, nb + 1, nb + 1}) d.take(c);
    CHECK(d.tiled() == nnodes * N + nb * n + nb + 3 * (nb + 1) + 2 * (nb + 1) * n);
  }
  {  // asset_hip_mesh_error_integrator: traj | abs | rel | xend | e | tsnd | errors | dist | error_max | dist_max | max_err; steps | status
    Layout<double> d;
    Layout<int> i;
    for (size_t c : {nnodes * N, n, n, nint * n, nint * n, nb + 1, (nb + 1) * n, (nb + 1) * n, nb + 1, nb + 1, size_t(1)}) d.take(c);
    for (size_t c : {nint * 2, nint}) i.take(c);
    CHECK(d.tiled() == nnodes * N + 2 * n + 2 * nint * n + 3 * (nb + 1) + 2 * (nb + 1) * n + 1 && i.tiled() == nint * 3);
  }
  for (int ctrl = 0; ctrl < 2; ctrl++)
    for (int stm = 0; stm < 2; stm++) {  // asset_hip_propagate* / _ctrl*: y0 | tf | abs | rel | xs | (us) | (stm: S | jac | xlast); steps | status
      const size_t nsu = stm ? 1 : ns, C = ctrl ? n + pv : N - 1, per = stm ? m * n : 0;
      Layout<double> d;
      Layout<int> i;
      for (size_t c : {m * N, m, n, n, m * nsu * n, ctrl ? m * nsu * uv : 0, per * C, per * (N + 1), per}) d.take(c);
      for (size_t c : {m * 2, m}) i.take(c);
      CHECK(d.tiled() == m * N + m + 2 * n + m * nsu * n + (ctrl ? m * nsu * uv : 0) + per * (C + N + 2) && i.tiled() == m * 3);
    }
  {  // asset_hip_propagate_events: y0 | tf | abs | rel | xf | t_end | ev_rows | ev_resid; steps | status | stopped | ev_count | ev_conv
    Layout<double> d;
    Layout<int> i;
    const size_t occ = m * ne * locs;
    for (size_t c : {m * N, m, n, n, m * n, m, occ * (n + 1), occ}) d.take(c);
    for (size_t c : {m * 2, m, m, m * ne, occ}) i.take(c);
    CHECK(d.tiled() == m * N + m + 2 * n + m * n + m + occ * (n + 2) && i.tiled() == m * 4 + m * ne + occ);
  }
  std::printf("ok\n");
  return 0;
}
"""


def test_arena_offsets_totals_and_the_layouts_of_the_entry_points(tmp_path):
    src, exe = tmp_path / "arena.cpp", tmp_path / "arena"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "asset_asrl_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr

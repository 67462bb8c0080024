// LsdOwned (lsd_slam_amd/csrc/owned.hpp) with fake release functions that count their calls: each case prints "ok" or the first thing
// that went wrong, and every case ends with nothing live and nothing released twice.  Stand-alone: built with the address and
// undefined-behaviour sanitizers by tests/test_owned_cpu.py.  Usage: owned_test <case> [n]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../lsd_slam_amd/csrc/owned.hpp"

static std::map<int*, int> g_released;     // value -> times released
static int g_handlesReleased = 0;
struct FakeFree { static void call(void* p) { g_released[(int*)p]++; } };
struct FakeHandleClose { static void call(long h) { g_handlesReleased += (int)h; } };   // an opaque non-pointer handle
using Ptr = LsdOwned<int*, FakeFree>;
using Handle = LsdOwned<long, FakeHandleClose>;
static long long live() { return LsdLive<FakeFree>::count.load(); }

static int g_storage[64];
static int* val(int i) { return &g_storage[i]; }
static int times(int i) { return g_released.count(val(i)) ? g_released[val(i)] : 0; }

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int case_destructor() {
  { Ptr a(val(0)); CHECK(live() == 1 && a.get() == val(0) && a && times(0) == 0); int* raw = a; CHECK(raw == val(0)); }
  CHECK(times(0) == 1 && live() == 0);
  { Ptr empty; CHECK(!empty && empty.get() == nullptr); }
  CHECK(g_released.size() == 1);      // an empty owner releases nothing
  { Handle h(7); CHECK(h && (long)h == 7 && LsdLive<FakeHandleClose>::count.load() == 1); }
  CHECK(g_handlesReleased == 7 && LsdLive<FakeHandleClose>::count.load() == 0);
  return 0;
}
static int case_move() {
  {
    Ptr a(val(1));
    Ptr b(std::move(a));
    CHECK(!a && a.get() == nullptr && b.get() == val(1) && live() == 1 && times(1) == 0);
    Ptr c;
    c = std::move(b);
    CHECK(!b && c.get() == val(1) && live() == 1 && times(1) == 0);
  }
  CHECK(times(1) == 1 && live() == 0);
  return 0;
}
static int case_move_assign_over_live() {
  {
    Ptr a(val(2)), b(val(3));
    CHECK(live() == 2);
    a = std::move(b);
    CHECK(times(2) == 1 && times(3) == 0 && a.get() == val(3) && !b && live() == 1);
    a.reset(val(4));
    CHECK(times(3) == 1 && a.get() == val(4) && live() == 1);
    a.reset();
    CHECK(times(4) == 1 && !a && live() == 0);
  }
  CHECK(times(2) == 1 && times(3) == 1 && times(4) == 1 && live() == 0);
  return 0;
}
static int case_self_move() {
  {
    Ptr a(val(5));
    Ptr& same = a;
    a = std::move(same);
    CHECK(a.get() == val(5) && times(5) == 0 && live() == 1);
  }
  CHECK(times(5) == 1 && live() == 0);
  return 0;
}
static int case_release() {
  int* raw = nullptr;
  {
    Ptr a(val(6));
    raw = a.release();
    CHECK(raw == val(6) && !a && live() == 0);
  }
  CHECK(times(6) == 0 && live() == 0);     // handed over: the owner never freed it
  { Ptr again(raw); CHECK(live() == 1); }
  CHECK(times(6) == 1 && live() == 0);
  return 0;
}
static int case_vector() {
  {
    std::vector<Ptr> v;     // grows from no capacity: several reallocations move the owners
    for (int i = 0; i < 40; i++) v.push_back(Ptr(val(i)));
    CHECK(live() == 40 && g_released.empty());
    for (int i = 0; i < 40; i++) CHECK(v[(size_t)i].get() == val(i));
    Ptr last = std::move(v.back());     // a frame takes an arena out of the pool
    v.pop_back();
    CHECK(last.get() == val(39) && live() == 40 && g_released.empty());
    v.erase(v.begin());
    CHECK(times(0) == 1 && live() == 39);
  }
  for (int i = 0; i < 40; i++) CHECK(times(i) == 1);
  CHECK(live() == 0);
  return 0;
}
// A creator in the library's pattern: the object in a unique_ptr, every resource in an owner member from the line that acquires it, the
// object released to the caller on the last line.  Step k (0-based) fails when k == failAt.
struct Model { Ptr step[8]; };
static int model_create(int n, int failAt, Model** out) {
  std::unique_ptr<Model> m(new Model());
  for (int k = 0; k < n; k++) {
    if (k == failAt) return -1;
    m->step[k].reset(val(k));
  }
  *out = m.release();
  return 0;
}
static int case_creator(int n) {
  CHECK(n >= 1 && n <= 8);
  for (int k = 0; k < n; k++) {
    g_released.clear();
    Model* out = (Model*)0x1;      // a refused call leaves *out untouched
    CHECK(model_create(n, k, &out) == -1 && out == (Model*)0x1);
    for (int i = 0; i < n; i++) CHECK(times(i) == (i < k ? 1 : 0));     // what was acquired before step k: released exactly once
    CHECK(live() == 0);
  }
  g_released.clear();
  Model* m = nullptr;
  CHECK(model_create(n, -1, &m) == 0 && m && live() == n && g_released.empty());
  delete m;
  for (int i = 0; i < n; i++) CHECK(times(i) == 1);
  CHECK(live() == 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string c = argv[1];
  int rc = 2;
  if (c == "destructor") rc = case_destructor();
  else if (c == "move") rc = case_move();
  else if (c == "move_assign_over_live") rc = case_move_assign_over_live();
  else if (c == "self_move") rc = case_self_move();
  else if (c == "release") rc = case_release();
  else if (c == "vector") rc = case_vector();
  else if (c == "creator" && argc > 2) rc = case_creator(std::atoi(argv[2]));
  if (rc == 0) {
    for (const auto& kv : g_released) if (kv.second != 1) { std::printf("FAILED: a value was released %d times\n", kv.second); return 1; }
    if (live() != 0) { std::printf("FAILED: %lld values still live\n", live()); return 1; }
    std::printf("ok\n");
  }
  return rc;
}

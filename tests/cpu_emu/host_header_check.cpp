// TEST INFRASTRUCTURE ONLY — a stand-alone program for mettagrid_amd/csrc/mgx_host.h on the emulated HIP runtime of this
// directory, built with AddressSanitizer + UndefinedBehaviorSanitizer and run by tests/test_host_header.py:
//   clang++ -std=c++17 -fsanitize=address,undefined -DMGX_CPU_EMU -I tests/cpu_emu -I include -I mettagrid_amd/csrc
//           tests/cpu_emu/host_header_check.cpp -pthread
// Exit status 0 and "host header ok" when every rule below holds.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "mgx_host.h"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

static std::atomic<int> g_failed{0};
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); g_failed++; } \
  } while (0)

static void kernel_a() {}
static void kernel_b() {}
static void kernel_c() {}

static void check_lds_limit() {
  const void* A = (const void*)kernel_a;
  const void* B = (const void*)kernel_b;
  MgxLdsLimit lim;
  // a larger request sets every kernel of the set
  CHECK(lim.raise({A, B}, 0, 70000) == hipSuccess);
  CHECK(emu_func_attr_calls == 2 && emu_func_attr[A] == 70000 && emu_func_attr[B] == 70000);
  // a smaller (or equal) one after it makes no attribute call and succeeds
  CHECK(lim.raise({A, B}, 0, 1000) == hipSuccess);
  CHECK(lim.raise({A, B}, 0, 70000) == hipSuccess);
  CHECK(emu_func_attr_calls == 2 && emu_func_attr[A] == 70000 && emu_func_attr[B] == 70000);
  CHECK(lim.raise({A, B}, 0, 70001) == hipSuccess);
  CHECK(emu_func_attr_calls == 4 && emu_func_attr[A] == 70001 && emu_func_attr[B] == 70001);
  // two devices keep separate maxima
  CHECK(lim.raise({A, B}, 1, 500) == hipSuccess);
  CHECK(emu_func_attr_calls == 6 && emu_func_attr[A] == 500);
  CHECK(lim.max_bytes[0] == 70001 && lim.max_bytes[1] == 500);
  CHECK(lim.raise({A, B}, 1, 400) == hipSuccess && emu_func_attr_calls == 6);
  // an ordinal outside the table is refused, without a call
  CHECK(lim.raise({A, B}, 64, 1 << 20) == hipErrorInvalidDevice);
  CHECK(lim.raise({A, B}, -1, 1 << 20) == hipErrorInvalidDevice);
  CHECK(emu_func_attr_calls == 6);
  // the units' form: the current device's maximum
  emu_current_device = 5;
  CHECK(lim.raise_current({A}, 300) && lim.max_bytes[5] == 300 && emu_func_attr[A] == 300);
  emu_current_device = 64;
  CHECK(!lim.raise_current({A}, 300));
  emu_current_device = 0;
  // eight threads raising concurrently end with the largest value recorded
  MgxLdsLimit shared;
  const void* C = (const void*)kernel_c;
  std::vector<std::thread> threads;
  for (int t = 0; t < 8; t++)
    threads.emplace_back([&shared, C, t] {
      for (int i = 0; i < 2000; i++) {
        const size_t bytes = (size_t)((i * 8 + (t * 3 + i) % 8) * 16);   // interleaved: every thread is overtaken again and again
        if (shared.raise({C}, 2, bytes) != hipSuccess) g_failed++;
      }
      if (shared.raise({C}, 2, (size_t)(1000000 + t)) != hipSuccess) g_failed++;
    });
  for (std::thread& th : threads) th.join();
  CHECK(shared.max_bytes[2] == 1000007 && emu_func_attr[C] == 1000007);
}

static void check_dev_image() {
  MgxDev d;
  memset(&d, 0, sizeof d);
  d.E = 7;
  MgxDevImage img;
  CHECK(img.differs(d));    // first use: nothing uploaded yet
  CHECK(!img.differs(d));   // the same table again
  d.max_steps = 9;          // one changed field
  CHECK(img.differs(d));
  CHECK(!img.differs(d) && img.host.max_steps == 9 && img.host.E == 7);

  // the constant-memory helper on top of it: uploads on first use and on change only, per device
  static MgxDev symbol;
  memset(&symbol, 0, sizeof symbol);
  MgxConstDev cd;
  { auto lock = cd.upload(&symbol, d, nullptr, "check"); CHECK(lock.owns_lock() && symbol.max_steps == 9); }
  symbol.max_steps = -1;    // (an upload would overwrite this)
  { auto lock = cd.upload(&symbol, d, nullptr, "check"); CHECK(symbol.max_steps == -1); }
  d.max_steps = 11;
  { auto lock = cd.upload(&symbol, d, nullptr, "check"); CHECK(symbol.max_steps == 11); }
  emu_current_device = 1;   // another device's symbol has not seen the table yet
  symbol.max_steps = -1;
  { auto lock = cd.upload(&symbol, d, nullptr, "check"); CHECK(symbol.max_steps == 11); }
  emu_current_device = 0;
  CHECK(mgx_pow2_at_least(1) == 1 && mgx_pow2_at_least(16) == 16 && mgx_pow2_at_least(17) == 32);
}

int main() {
  check_lds_limit();
  check_dev_image();
  if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed.load()); return 1; }
  printf("host header ok\n");
  return 0;
}

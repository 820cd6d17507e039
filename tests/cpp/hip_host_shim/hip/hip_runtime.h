// Stand-in for <hip/hip_runtime.h> that lets a kernel source compile as plain C++ and run on the host, one std::thread per GPU thread
// (tests/cpp/png_kernels_host.cpp).  A workgroup is `block` host threads; __syncthreads is a barrier over them; __shared__ variables are
// function-local statics, shared by the threads of the one workgroup that runs at a time.  Only what the kernels under test use is here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <barrier>
#include <thread>
#include <vector>

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct float2 { float x, y; };
typedef struct host_shim_stream* hipStream_t;
typedef struct host_shim_event* hipEvent_t;

inline thread_local dim3 threadIdx, blockIdx, gridDim;
inline std::barrier<>* host_shim_barrier = nullptr;

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static
#define hipLaunchKernelGGL(...) ((void)0)   /* the launch wrappers compile; the harness calls the kernels itself */

inline void __syncthreads() { host_shim_barrier->arrive_and_wait(); }
inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
inline unsigned __brev(unsigned v) {
  unsigned r = 0;
  for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
  return r;
}
using std::max;
using std::min;

// one workgroup after the other, `block` host threads each
template <class Kernel, class... Args>
void host_shim_launch(Kernel kernel, unsigned grid, unsigned block, Args... args) {
  std::barrier<> bar(block);
  host_shim_barrier = &bar;
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < block; ++t)
    threads.emplace_back([=, &bar]() {
      threadIdx = dim3(t); gridDim = dim3(grid);
      // the same host threads run workgroup after workgroup (a grid of a thousand small workgroups would otherwise spend its time starting
      // threads); the barrier between two keeps a workgroup's __shared__ statics its own until its last thread is done
      for (unsigned b = 0; b < grid; ++b) { blockIdx = dim3(b); kernel(args...); bar.arrive_and_wait(); }
    });
  for (auto& th : threads) th.join();
}

#pragma once
// What csrc/optim.hip needs beyond tools/fcstack_host/hip/hip_runtime.h (the shim that runs a launch on std::threads): the
// agent-scope atomics and the fence of the last-arriver hand-off, as the compiler's own host atomics.
#include <cmath>
#include <cstdint>
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_fetch_add(ptr, val, order, scope) __atomic_fetch_add(ptr, val, order)
#define __hip_atomic_store(ptr, val, order, scope) __atomic_store_n(ptr, val, order)
#define __builtin_amdgcn_fence(order, scope) __atomic_thread_fence(order)

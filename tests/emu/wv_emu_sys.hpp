// wv_emu_sys.hpp — the CPU twins of swp_wave.hpp's system-scope primitives (sys_fence, sys_store32, sys_store_release32, sys_load32:
// the words a host polls while a kernel runs), next to wv_emu.hpp, which stays as it is for the programs that do not need them.
//
// TEST INFRASTRUCTURE. The fibers run on one thread, so a store is visible at once and a fence is nothing; what a test wants is to stand
// where the polling host stands: emu::sys_release_hook() is called at every release store, with the word and its new value — everything
// the kernel stored in front of it must be in place by then. (The hook runs on the storing fiber: it must not call a collective.)
#pragma once
#include "wv_emu.hpp"

namespace emu {
inline std::function<void(const u32*, u32)>& sys_release_hook() {
    static std::function<void(const u32*, u32)> h;
    return h;
}
}  // namespace emu

namespace wv {
inline void sys_fence() {}
inline void sys_store32(u32* p, u32 v) { *reinterpret_cast<volatile u32*>(p) = v; }
inline void sys_store_release32(u32* p, u32 v) {
    *reinterpret_cast<volatile u32*>(p) = v;
    if (emu::sys_release_hook()) emu::sys_release_hook()(p, v);
}
inline u32 sys_load32(const u32* p) { return *reinterpret_cast<const volatile u32*>(p); }
}  // namespace wv

// Host-side state every launcher shares: cached environment knobs, the dynamic-LDS opt-in and the CU count.  Nothing here is device
// code (common.h is the device helpers' file).  What a launcher may rely on: the opt-in and the CU count belong to the device that is
// current at the call, first calls may come from several host threads at once, and the steady state is one hipGetDevice and one atomic
// load — no lock, no allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <mutex>

// An integer knob from the environment.  Call sites cache it for the process: `static const int x = env_int("GECCO_...", dflt);`
// (a thread-safe initialisation), and validate or clamp the cached value themselves.
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// GECCO_TN_XCD=0: plain dispatch order in the weight-gradient GEMMs (A/B runs)
inline int tn_xcd() {
    static const int v = env_int("GECCO_TN_XCD", 1) != 0;
    return v;
}

constexpr int LAUNCH_MAX_DEVICES = 64;   // ordinals past it are served without the caches
inline std::mutex g_launch_state_mutex;  // first calls only

inline std::atomic<int>* device_slot(std::atomic<int>* per_device, int* dev) {
    *dev = 0;
    (void)hipGetDevice(dev);
    return *dev >= 0 && *dev < LAUNCH_MAX_DEVICES ? per_device + *dev : nullptr;
}

// Lets `Kernels` (the instantiations one launcher picks among) use `bytes` of dynamic LDS on the current device.  The state is keyed by
// the kernels and the device; hipFuncSetAttribute runs only when `bytes` exceeds what that device has granted them so far.  A launcher
// returns a failure to its caller instead of launching.
template <auto... Kernels>
hipError_t lds_opt_in(size_t bytes) {
    static std::atomic<int> granted[LAUNCH_MAX_DEVICES] = {};
    int dev;
    std::atomic<int>* const slot = device_slot(granted, &dev);
    if (slot && (int)bytes <= slot->load(std::memory_order_acquire)) return hipSuccess;
    std::lock_guard<std::mutex> lock(g_launch_state_mutex);   // a smaller request never undoes a larger one granted meanwhile
    if (slot && (int)bytes <= slot->load(std::memory_order_relaxed)) return hipSuccess;
    for (const void* k : {reinterpret_cast<const void*>(Kernels)...}) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    if (slot) slot->store((int)bytes, std::memory_order_release);
    return hipSuccess;
}

// Compute units of the current device; 256 when the query fails.
inline int device_cus() {
    static std::atomic<int> cus[LAUNCH_MAX_DEVICES] = {};
    int dev, n = 0;
    std::atomic<int>* const slot = device_slot(cus, &dev);
    if (slot && (n = slot->load(std::memory_order_relaxed)) > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    if (slot) slot->store(n, std::memory_order_relaxed);
    return n;
}

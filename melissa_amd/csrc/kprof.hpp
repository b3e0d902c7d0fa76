// In-kernel cycle profilers: one lap timer for every instrumented kernel family, and one way to read its counters.
//
// A family is a device array of counters next to its kernel (one comment line per slot there) and a compile-time switch
// derived from its -DMEL_*_PROF flag.  The kernel holds a KLaps<ON, SLOTS>: with ON = false that is an empty struct whose
// members are empty functions, so an ordinary build carries no trace of it; with ON = true it keeps SLOTS cycle sums and the
// last stamp in registers and adds them to the family's array once, at flush().  Hosts read (and zero) a family through
// mel_debug_prof_read(family, out, cap) (fwd.hip); tools/kprof.py wraps that.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mel {

enum KprofFamily {
    KPROF_WORLD = 0,   // MEL_ENV_PROF       env.hip        world_step
    KPROF_ENV = 1,     // MEL_ENV_PROF       env.hip        env_round_kernel
    KPROF_GEMM = 2,    // MEL_GEMM_PROF=tag  gemm_f32.hpp   persistent kernel (MEL_SPLIT_PROF: the 128 x 128 split kernel)
    KPROF_SPLIT = 3,   // MEL_SPLIT_PROF     gemm_split.hpp stamps inside a K step of the 128 x 128 split kernel
    KPROF_RING = 4,    // MEL_RING_PROF=tag  gemm_ring.hpp
    KPROF_TABLE = 5,   // MEL_TABLE_PROF     gemm_table.hpp
    KPROF_ATT = 6,     // MEL_ATT_PROF=mode  attention.hpp  rows kernel
    KPROF_FIN = 7,     // MEL_FIN_PROF       heads.hpp      head_finish_kernel
    KPROF_FAMILIES
};

// A pin keeps the stamp that follows behind the computation of a value: kpin(x) for a value in vector registers,
// kpin(ksgpr(x)) for a wave-uniform one.
template <class T>
struct KSgpr {
    T x;
};
template <class T>
__device__ __forceinline__ KSgpr<T> ksgpr(T x) {
    return {x};
}
template <class T>
__device__ __forceinline__ void kpin(T x) {
    asm volatile("s_nop 0" ::"v"(x));
}
template <class T>
__device__ __forceinline__ void kpin(KSgpr<T> p) {
    asm volatile("s_nop 0" ::"s"(p.x));
}

template <bool ON>
struct KStamp {};
template <>
struct KStamp<true> {
    unsigned long long t;
};

// ON = false: nothing.  (Static members: the calls do not even take the address of the empty object, so its presence cannot
// reorder anything in the kernel around it.)
template <bool ON, int SLOTS>
struct KLaps {
    using Stamp = KStamp<false>;
    template <class... P> static __device__ __forceinline__ Stamp mark(P...) { return {}; }
    template <class... P> static __device__ __forceinline__ Stamp mark_fenced(P...) { return {}; }
    template <class... P> static __device__ __forceinline__ Stamp lap(int, P...) { return {}; }
    template <class... P> static __device__ __forceinline__ Stamp lap_fenced(int, P...) { return {}; }
    template <class... P> static __device__ __forceinline__ Stamp since(int, Stamp, P...) { return {}; }
    template <class... P> static __device__ __forceinline__ Stamp since_fenced(int, Stamp, P...) { return {}; }
    static __device__ __forceinline__ void add(int, unsigned long long) {}
    static __device__ __forceinline__ void wait_lds() {}
    static __device__ __forceinline__ void wait_vmem() {}
    static __device__ __forceinline__ void flush(unsigned long long*, bool) {}
};

template <int SLOTS>
struct KLaps<true, SLOTS> {
    using Stamp = KStamp<true>;
    unsigned long long v[SLOTS] = {}, last = 0;

    // begin a lap here (what passed since the previous stamp is charged to no slot)
    template <class... P> __device__ __forceinline__ Stamp mark(P... pins) { return now<false>(pins...); }
    template <class... P> __device__ __forceinline__ Stamp mark_fenced(P... pins) { return now<true>(pins...); }
    // slot += cycles since the previous stamp
    template <class... P> __device__ __forceinline__ Stamp lap(int slot, P... pins) { return since(slot, Stamp{last}, pins...); }
    template <class... P> __device__ __forceinline__ Stamp lap_fenced(int slot, P... pins) { return since_fenced(slot, Stamp{last}, pins...); }
    // slot += cycles since an earlier stamp (a span around inner laps, the whole kernel)
    template <class... P> __device__ __forceinline__ Stamp since(int slot, Stamp from, P... pins) {
        const Stamp s = now<false>(pins...);
        add(slot, s.t - from.t);
        return s;
    }
    // ... with the stamp fenced off from the scheduler on both sides (stamps between the MFMA groups of one K step)
    template <class... P> __device__ __forceinline__ Stamp since_fenced(int slot, Stamp from, P... pins) {
        const Stamp s = now<true>(pins...);
        add(slot, s.t - from.t);
        return s;
    }
    // event counts: samples, K steps, rows, loop iterations.  (Selects, not an indexed store: a slot chosen at run time must
    // not move the sums out of registers; a constant slot folds to one addition.)
    __device__ __forceinline__ void add(int slot, unsigned long long value) {
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) v[i] += i == slot ? value : 0ull;
    }
    // what the next stamp should include: this wave's LDS operations / its global loads and stores have completed
    __device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
    __device__ __forceinline__ void wait_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    // one lane of the sampled waves adds every slot to the family's counters
    __device__ __forceinline__ void flush(unsigned long long* counters, bool sampled) {
        if (sampled)
            for (int i = 0; i < SLOTS; ++i) atomicAdd(&counters[i], v[i]);
    }

private:
    template <bool FENCED, class... P> __device__ __forceinline__ Stamp now(P... pins) {
        if (FENCED) __builtin_amdgcn_sched_barrier(0);
        (kpin(pins), ...);
        last = __builtin_readcyclecounter();
        if (FENCED) __builtin_amdgcn_sched_barrier(0);
        return Stamp{last};
    }
};

// Host side: read and zero a family's counter array.  Returns its slot count, 0 if this build does not instrument it.
template <int N>
static inline int32_t kprof_read(bool on, unsigned long long (&counters)[N], unsigned long long* out, int32_t cap) {
    if (!on) return 0;
    unsigned long long got[N], zero[N] = {};
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(got, HIP_SYMBOL(counters), sizeof(got));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(counters), zero, sizeof(zero));
    for (int i = 0; i < N && i < cap; ++i) out[i] = got[i];
    return N;
}
int32_t kprof_read_env(int32_t family, unsigned long long* out, int32_t cap);      // the families of env.hip

}  // namespace mel

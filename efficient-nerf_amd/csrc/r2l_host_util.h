// Host helpers shared by the C-ABI files: error reporting, number formats, and the two owners of device state (DevBuf, EventTimer)
// that let a context clean up after itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <vector>

#include "../../include/r2l_hip.h"
#include "r2l_common.h"

int r2l_set_error(int code, const char* fmt, ...);
int r2l_require_gfx950(int* n_cu);
void r2l_linspace01(int steps, float* out);                        // torch.linspace(0,1,steps), f32
void r2l_z_vals(int steps, float near_, float far_, float* out);  // near*(1-t)+far*t, f32 per-op rounding
float r2l_pow2_scale(const float* w, size_t n);                    // 2^e with max|w|*2^e in [2^12,2^13)
void r2l_split_f16(float v, _Float16* hi, _Float16* lo);
unsigned char r2l_f32_to_e4m3(float v);                            // OCP e4m3fn, round-to-nearest-even, saturating
int r2l_layer_exponent(const float* w, size_t n);                  // e with max|w| in [2^(e-1), 2^e); -4 for all-zero
unsigned r2l_f_to_bf6(double v);                                   // OCP bf6 = e3m2 code, round-to-nearest-even, saturating

#define HIPCHK(call, what)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return r2l_set_error(R2L_EHIP, what ": %s", hipGetErrorString(e_)); \
    } while (0)

// fp16 parts per weight of the compiler-scheduled chunk stream (r2l_common.h): hi alone, or hi | lo
static inline int np_of(int mode) { return mode == R2L_PREC_FP16X1 ? 1 : 2; }

// element j of `lane` in fragment `frag` of a chunk of that stream
static inline void put_frag(char* chunk, int np, int frag, int lane, int j, float v) {
    _Float16 hi, lo;
    r2l_split_f16(v, &hi, np == 2 ? &lo : nullptr);
    reinterpret_cast<_Float16*>(chunk + (size_t)(frag * np + 0) * R2L_FRAG_BYTES + lane * 16)[j] = hi;
    if (np == 2) reinterpret_cast<_Float16*>(chunk + (size_t)(frag * np + 1) * R2L_FRAG_BYTES + lane * 16)[j] = lo;
}

// Device memory with one owner.  Reads like the pointer it holds; empty until grow() or upload() succeeds and empty again after either
// fails.  The destructor makes no runtime call for an empty buffer (contexts die in Python's __del__, possibly at interpreter
// shutdown, and the host-only sanitizer build leaves the runtime unresolved) and ignores the error of the call it does make.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t size() const { return n_; }      // elements

    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // room for n elements; what is there already stays when it is enough.  Frees BEFORE it allocates: the peak never holds both
    int grow(size_t n, const char* what) {
        if (n <= n_) return R2L_OK;
        release();
        hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return r2l_set_error(R2L_EHIP, "%s: %s", what, hipGetErrorString(e));
        }
        n_ = n;
        return R2L_OK;
    }
    // a NEW allocation of n + room elements with the first n copied from the host.  Whatever was held is freed first, and hipFree
    // waits for the device: no launch in flight reads the old bytes or sees the new ones half written
    int upload(const T* src, size_t n, const char* what, size_t room = 0) {
        release();
        int rc = grow(n + room, what);
        if (rc) return rc;
        hipError_t e = hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) return R2L_OK;
        release();
        return r2l_set_error(R2L_EHIP, "%s: %s", what, hipGetErrorString(e));
    }
};

// HIP-event timing of the dominant launches (*_timing_enable / *_kernel_time_ms): a pool of start / stop pairs, made on demand,
// recorded on the stream the launch goes to
class EventTimer {
    std::vector<hipEvent_t> ev_;      // pairs
    size_t used_ = 0;

public:
    bool on = false;
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
    ~EventTimer() {
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    }
    // the next pair: its start goes onto s now, its stop with stop(); both do nothing while the timer is off
    int start(hipStream_t s) {
        if (!on) return R2L_OK;
        while (used_ + 2 > ev_.size()) {
            hipEvent_t e;
            hipError_t er = hipEventCreate(&e);
            if (er != hipSuccess) return r2l_set_error(R2L_EHIP, "hipEventCreate: %s", hipGetErrorString(er));
            ev_.push_back(e);
        }
        used_ += 2;
        (void)hipEventRecord(ev_[used_ - 2], s);
        return R2L_OK;
    }
    void stop(hipStream_t s) {
        if (on) (void)hipEventRecord(ev_[used_ - 1], s);
    }
    // waits for every pair handed out since the last reset
    int total(double* total_ms, int* n_pairs, int reset) {
        double tot = 0;
        for (size_t i = 0; i + 1 < used_; i += 2) {
            float ms = 0;
            hipError_t e = hipEventSynchronize(ev_[i + 1]);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]);
            if (e != hipSuccess) return r2l_set_error(R2L_EHIP, "event timing: %s", hipGetErrorString(e));
            tot += ms;
        }
        if (total_ms) *total_ms = tot;
        if (n_pairs) *n_pairs = (int)(used_ / 2);
        if (reset) used_ = 0;
        return R2L_OK;
    }
};

// Persistent workgroups take ray tiles b, b + grid, ...: with one workgroup per CU the launch lasts ceil(n_tiles / n_cu) tile
// times and the last round is partly empty (5,000 tiles on 256 CUs: 19.5 rounds).  The smallest grid with the same number of
// rounds gives every workgroup the same work and leaves the idle CUs' share of the package power to the others: 250 workgroups
// for 5,000 tiles, -1.3 % kernel time (256 -> 250 same-call A/B; 228 = 22 rounds +0.9 %, 200 = 25 rounds +3.9 %).
#ifdef R2L_GRID_OVERRIDE      // experiment (tools/build_variant.sh CAPI_DEF=-DR2L_GRID_OVERRIDE=250)
static inline int balanced_grid(int n_tiles, int) { return n_tiles < R2L_GRID_OVERRIDE ? n_tiles : R2L_GRID_OVERRIDE; }
#else
static inline int balanced_grid(int n_tiles, int n_cu) {
    if (n_tiles <= n_cu) return n_tiles;
    const int rounds = (n_tiles + n_cu - 1) / n_cu;
    return (n_tiles + rounds - 1) / rounds;
}
#endif

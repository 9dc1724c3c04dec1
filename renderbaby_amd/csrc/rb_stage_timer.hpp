// rb_stage_timer.hpp -- the kernel time of one stage on a stream: event pairs recorded round the stage's launches, read when
// somebody asks.  Host code only; every member that touches an event wants the events' device current.
#pragma once
#include <hip/hip_runtime_api.h>

#include <vector>

namespace rb {

struct __attribute__((visibility("hidden"))) StageTimer {   // (the library's dynamic symbols stay what they were)
    std::vector<hipEvent_t> ev;   // begin, end per pair; made when first needed and kept until destroy()
    size_t pairs = 0;             // pairs recorded and not yet folded into `ms`
    float ms = 0.0f;              // the folded time

    // the recorded pairs and the folded time are gone; no HIP call
    void reset() {
        pairs = 0;
        ms = 0.0f;
    }
    hipError_t begin(hipStream_t stream) {
        while (ev.size() < 2 * (pairs + 1)) {
            hipEvent_t x = nullptr;
            if (const hipError_t st = hipEventCreate(&x)) return st;
            ev.push_back(x);
        }
        return hipEventRecord(ev[2 * pairs], stream);
    }
    // counts the pair: a stage whose launch failed after begin() leaves nothing to read
    hipError_t end(hipStream_t stream) {
        const hipError_t st = hipEventRecord(ev[2 * pairs + 1], stream);
        if (st == hipSuccess) pairs++;
        return st;
    }
    // `fn()` queues the stage and returns a HIP status; the first bad status of the three steps
    template <class Fn>
    int timed(hipStream_t stream, Fn&& fn) {
        if (const hipError_t st = begin(stream)) return static_cast<int>(st);
        if (const int st = fn()) return st;
        return static_cast<int>(end(stream));
    }
    // The folded time, after the outstanding pairs are folded into it in the order they were recorded: waits for the last of
    // them.  A second read has nothing to wait for and gives the same value.
    hipError_t read(float* out) {
        if (pairs) {
            if (const hipError_t st = hipEventSynchronize(ev[2 * pairs - 1])) return st;
            float sum = ms;
            for (size_t i = 0; i < pairs; i++) {
                float pair_ms = 0.0f;
                if (const hipError_t st = hipEventElapsedTime(&pair_ms, ev[2 * i], ev[2 * i + 1])) return st;
                sum += pair_ms;
            }
            ms = sum;
            pairs = 0;
        }
        *out = ms;
        return hipSuccess;
    }
    void destroy() {
        for (hipEvent_t x : ev) (void)hipEventDestroy(x);
        ev.clear();
        pairs = 0;
    }
};

}  // namespace rb

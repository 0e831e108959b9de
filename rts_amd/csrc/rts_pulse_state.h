// rts_pulse_state.h -- the phase of a handle's pulse, and the count of pulses that share a device.  A handle's pulse is IDLE
// (nothing in flight), OPEN (begun: the trace is in flight) or CHAINED (closed to the caller: its post-processing was enqueued on
// the device-side received count and awaits its resolution).  A pulse that is not IDLE is counted on its device's slot, and the
// transitions below are the ONLY code that moves that count: a launch sizes its grid by it (rts_launch_plan.h: rts_trace_grid
// through shared_gpu), so a miscount would quietly change every later launch of the device.  No HIP, no handle: it compiles
// with any host compiler and is tested without a GPU (tests/test_pulse_state_host.py).
#pragma once
#include <atomic>

#define RTS_PULSE_SLOTS 64          // devices share a slot modulo this
// the slot of a device in an array of RTS_PULSE_SLOTS counters (atomic: handles may be driven from different threads)
inline std::atomic<int>& rts_pulse_slot(std::atomic<int>* counters, int device) { return counters[device & (RTS_PULSE_SLOTS - 1)]; }

//   transition   from -> to           count
//   begin        IDLE -> OPEN         +1      on the slot it is given; the later transitions give back what it took
//   end          OPEN -> IDLE         -1
//   chain        OPEN -> CHAINED       0      (a chained pulse's kernels still share the device)
//   resolve      CHAINED -> IDLE      -1
//   abandon      any -> IDLE          -1 unless already IDLE
// A transition from another phase changes nothing and returns false.
class RtsPulseState {
public:
    bool idle() const { return phase_ == IDLE; }
    bool open() const { return phase_ == OPEN; }
    bool chained() const { return phase_ == CHAINED; }
    bool begin(std::atomic<int>& slot) { if (phase_ != IDLE) return false; phase_ = OPEN; slot_ = &slot; slot_->fetch_add(1); return true; }
    bool end() { return phase_ == OPEN && leave(); }
    bool chain() { if (phase_ != OPEN) return false; phase_ = CHAINED; return true; }
    bool resolve() { return phase_ == CHAINED && leave(); }
    bool abandon() { return phase_ != IDLE && leave(); }
private:
    enum Phase { IDLE, OPEN, CHAINED };
    bool leave() { phase_ = IDLE; slot_->fetch_sub(1); slot_ = nullptr; return true; }
    Phase phase_ = IDLE;
    std::atomic<int>* slot_ = nullptr;      // the slot this pulse is counted on; null exactly when IDLE
};

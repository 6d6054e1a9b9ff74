// Process-wide host state of the launchers: the live kernel timing, and the per-device caches of the
// GEMM launch helpers (gemm_launch.hpp). Host code only.
#include "gm2_kernels.hpp"

#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace gm2 {

// ------------------------------------------------------------------------------------------------
// live timing of one kernel class (bench.py's roofline leg): event pairs on the launch stream
// ------------------------------------------------------------------------------------------------
namespace {
struct TimingState {
  int classes = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  std::vector<int> cls;  // the class of each used event pair
  size_t used = 0;
  std::map<int, std::pair<double, int64_t>> last;  // per-class totals of the last timed region
};
TimingState& tstate() {
  static TimingState t;
  return t;
}
}  // namespace

void timing_begin(int classes) {
  TimingState& t = tstate();
  t.classes = classes;
  t.used = 0;
}

void timing_end(double* total_ms, int64_t* launches) {
  TimingState& t = tstate();
  double tot = 0.0;
  t.last.clear();
  for (size_t i = 0; i < t.used; ++i) {
    hipError_t e = hipEventSynchronize(t.ev[i].second);
    if (e != hipSuccess) throw Gm2Error("timing: %s", hipGetErrorString(e));
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, t.ev[i].first, t.ev[i].second);
    if (e != hipSuccess) throw Gm2Error("timing: %s", hipGetErrorString(e));
    tot += ms;
    auto& l = t.last[t.cls[i]];
    l.first += ms;
    l.second += 1;
  }
  *total_ms = tot;
  *launches = (int64_t)t.used;
  t.classes = 0;
  t.used = 0;
}

void timing_class(int cls, double* total_ms, int64_t* launches) {
  const TimingState& t = tstate();
  auto it = t.last.find(cls);
  *total_ms = it == t.last.end() ? 0.0 : it->second.first;
  *launches = it == t.last.end() ? 0 : it->second.second;
}

TimedLaunch::TimedLaunch(int c, hipStream_t st) : idx(-1), s(st), cls(c) {
  TimingState& t = tstate();
  if (!(t.classes & cls)) return;
  if (t.used == t.ev.size()) {
    hipEvent_t a, b;
    // (device-scope release: no L2 write-back around the timed kernel)
    if (hipEventCreateWithFlags(&a, hipEventReleaseToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&b, hipEventReleaseToDevice) != hipSuccess)
      throw Gm2Error("hipEventCreate");
    t.ev.push_back({a, b});
  }
  idx = (int)t.used++;
  if (t.cls.size() < t.used) t.cls.resize(t.used);
  t.cls[idx] = cls;
  if (hipEventRecord(t.ev[idx].first, s) != hipSuccess) throw Gm2Error("hipEventRecord");
}

TimedLaunch::~TimedLaunch() {
  if (idx >= 0) (void)hipEventRecord(tstate().ev[idx].second, s);
}

// ------------------------------------------------------------------------------------------------
// per-device caches of the GEMM launch helpers: one copy for every translation unit
// ------------------------------------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is per device: remember (device, kernel) pairs
void ensure_lds_attr(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) throw Gm2Error("hipGetDevice");
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({dev, fn})) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
    throw Gm2Error("hipFuncSetAttribute(MaxDynamicSharedMemorySize=%d)", bytes);
  done.insert({dev, fn});
}

// compute units of the current device (cached per device)
int device_cus() {
  static std::mutex mu;
  static std::map<int, int> cus;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) throw Gm2Error("hipGetDevice");
  std::lock_guard<std::mutex> lk(mu);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    throw Gm2Error("hipDeviceGetAttribute(MultiprocessorCount)");
  return cus[dev] = std::max(n, 1);
}

}  // namespace gm2

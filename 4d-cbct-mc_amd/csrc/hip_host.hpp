#pragma once
// hip_host.hpp -- what the host code around the device routines shares (engine*.cpp, scan.cpp, fdk.hip, wpc_fit.hip, registration.hip,
// field_inverse.hip, shroud.hip, forward_project.hip, primary_project.hip, rooster4d.hip, resample.hip, speedup_net.hip, speedup_train.hip,
// segment_net.hip, segment_train.hip): the HIP check, the exception boundary of the C ABI, owners of HIP handles and of one call's device
// memory, the stage timer, the refusal of an argument, the block count of a one-thread-per-element launch, the host stopwatch, the reader
// of struct_size-versioned options, the writer of such reports and the small rules of the circular cone-beam geometry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host_model.hpp"  // mcgpu::Error, the only error type

namespace mcgpu {

int set_error(int code, const std::string& msg);  // engine.cpp: records the calling thread's last error, returns `code`
void require(bool ok, int code, const char* msg);  // model_device.cpp: throws Error(code, msg) unless ok

// The runtime also keeps a failed call's code as the thread's last error until hipGetLastError() takes it.  The check takes it, so
// a failure is reported once, to the call it belongs to, and not again by the launch check of the next, valid call on the thread.
#define HIP_TRY(expr)                                                                                          \
  do {                                                                                                         \
    hipError_t _e = (expr);                                                                                    \
    if (_e != hipSuccess) {                                                                                    \
      (void)hipGetLastError();                                                                                 \
      throw mcgpu::Error(-1, std::string("!!HIP ERROR!! ") + #expr + ": " + hipGetErrorString(_e));            \
    }                                                                                                          \
  } while (0)

// The body of every extern "C" function stands between these two: no exception leaves the C ABI
#define ABI_BEGIN try {
#define ABI_END                                                                     \
  }                                                                                 \
  catch (const mcgpu::Error& e) { return mcgpu::set_error(e.code, e.what()); }      \
  catch (const std::exception& e) { return mcgpu::set_error(-2, e.what()); }        \
  catch (...) { return mcgpu::set_error(-2, "unknown failure"); }

#pragma GCC visibility push(hidden)  // what follows is inline in every user: nothing of it joins the library's dynamic symbols

// A HIP object that remembers its device and is released there.  make(dev) hands the create call its out-parameter.
template <class T, hipError_t (*Release)(T)>
struct Owned {
  T h = nullptr;
  int dev = -1;
  Owned() = default;
  Owned(const Owned&) = delete;
  ~Owned() { reset(); }
  T* make(int device) { reset(); dev = device; return &h; }
  void reset() { if (h) { (void)hipSetDevice(dev); (void)Release(h); h = nullptr; } }
  operator T() const { return h; }
};
using DeviceBuffer = Owned<void*, hipFree>;
using PinnedBuffer = Owned<void*, hipHostFree>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// Device buffers and the timing events of one call, on the device that is current during it; frees everything it made, tracks the
// peak of the bytes it holds
struct CallDevice {
  std::vector<void*> bufs;
  std::vector<size_t> sizes;
  size_t held = 0, peak = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;  // what a Stage records
  CallDevice() = default;
  CallDevice(const CallDevice&) = delete;
  void events() {
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
  }
  template <class T>
  T* alloc(size_t bytes) {
    bufs.reserve(bufs.size() + 1);  // so that nothing can throw between hipMalloc and the owner's knowing of the buffer
    sizes.reserve(sizes.size() + 1);
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    bufs.push_back(p);
    sizes.push_back(bytes);
    held += bytes;
    peak = std::max(peak, held);
    return (T*)p;
  }
  template <class T>
  T* alloc_zeroed(size_t bytes) {
    T* p = alloc<T>(bytes);
    HIP_TRY(hipMemset(p, 0, bytes));
    return p;
  }
  template <class T>
  T* upload(const T* host, size_t n) {
    T* p = alloc<T>(n * sizeof(T));
    HIP_TRY(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
  template <class T>
  T* upload(const std::vector<T>& host) { return upload(host.data(), host.size()); }
  void release(void* p) {
    for (size_t i = 0; i < bufs.size(); ++i)
      if (bufs[i] == p) { (void)hipFree(p); held -= sizes[i]; bufs.erase(bufs.begin() + i); sizes.erase(sizes.begin() + i); return; }
  }
  ~CallDevice() {
    for (void* p : bufs) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

struct Stage {  // times a block of launches on the null stream into one report field
  CallDevice& dev;
  double& ms;
  Stage(CallDevice& d, double& m) : dev(d), ms(m) { HIP_TRY(hipEventRecord(dev.e0, nullptr)); }
  void done() {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(dev.e1, nullptr));
    HIP_TRY(hipEventSynchronize(dev.e1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, dev.e0, dev.e1));
    ms += t;
  }
};

// what an entry point throws at an argument or a size it does not take: the message the C ABI's callers see
[[noreturn]] inline void refuse(const char* fn, const std::string& what) { throw Error(-1, std::string("!!ERROR!! ") + fn + ": " + what); }

// blocks of 256 threads that cover n elements
inline unsigned int blocks_of(size_t n) { return (unsigned int)((n + 255) / 256); }

struct Stopwatch {  // host milliseconds since it was made: the uploads and whole calls that no Stage brackets
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Options structs of the C ABI begin with `unsigned int struct_size` and an int.  A caller built against an older header passes a
// shorter struct: what it does not have reads as zero.  Refused: no struct, or a size that does not reach past those two fields.
template <class T>
void read_options(const char* fn, const char* struct_name, const T* caller, T& out) {
  if (!caller || caller->struct_size < sizeof(unsigned int) + sizeof(int))
    throw Error(-1, std::string("!!ERROR!! ") + fn + ": set " + struct_name + ".struct_size = sizeof(" + struct_name + ")");
  memset(&out, 0, sizeof out);
  memcpy(&out, caller, std::min<size_t>(caller->struct_size, sizeof out));
  out.struct_size = (unsigned int)sizeof out;
}

// Reports of the C ABI that begin with `unsigned int struct_size` go back the other way: the caller gets the first
// min(its struct_size, sizeof) bytes of the filled report and keeps the struct_size it passed.  A null report is none wanted; one
// that does not reach past 8 bytes is refused before any work (`argument`: the parameter's name in the message).
template <class T>
void check_report(const char* fn, const char* argument, const char* struct_name, const T* caller) {
  if (caller && caller->struct_size < 8)
    throw Error(-1, std::string("!!ERROR!! ") + fn + ": set " + argument + "->struct_size = sizeof(" + struct_name + ")");
}
template <class T>
void write_report(T* caller, T filled) {
  if (!caller) return;
  filled.struct_size = (unsigned int)sizeof filled;
  const unsigned int want = caller->struct_size;  // as the caller was compiled
  memcpy(caller, &filled, std::min<size_t>(want, sizeof filled));
  caller->struct_size = want;
}

// ---- the circular cone-beam geometry of mcgpu_fdk_options, mcgpu_fp_options and mcgpu_rooster4d_options ----------------------
// origin of a volume axis (centre of voxel 0): NaN means centred
inline double centred_origin(int n, double spacing, double given) { return std::isnan(given) ? -(n - 1) / 2.0 * spacing : given; }
// detector offsets of projection p: an array that is not given reads as 0
template <class O>
double offset_x(const O& o, int p) { return o.proj_offset_x ? o.proj_offset_x[p] : 0.0; }
template <class O>
double offset_y(const O& o, int p) { return o.proj_offset_y ? o.proj_offset_y[p] : 0.0; }
// cos / sin of the gantry angle, detector offsets [mm].  Also a kernel argument (joseph_ray.inc: FpProj): its layout is the kernels'
struct ProjectionPose { double c, s, off_x, off_y; };
template <class O>
ProjectionPose projection_pose(const O& o, int p) {
  const double t = o.gantry_deg[p] * M_PI / 180.0;
  return {std::cos(t), std::sin(t), offset_x(o, p), offset_y(o, p)};
}

#pragma GCC visibility pop

}  // namespace mcgpu

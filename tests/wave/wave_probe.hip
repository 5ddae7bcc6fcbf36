// The group primitives of pink_amd/csrc/wave.h on the device's own code path -- TEST CODE ONLY: built by
// __graft_entry__.build() into tests/wave/libwaveprobe.so (its own library: libpinkhip's objects and exported names do not
// change), loaded by tests/test_wave_primitives.py.  The kernel body is wave_probe_kernel.h, shared with the CPU emulator.
#include "../../pink_amd/csrc/wave.h"
// clang-format off
#include "wave_probe_kernel.h"
// clang-format on

#include <cstdio>

namespace {

char g_error[256] = "";

template <int W>
__global__ __launch_bounds__(pinkhip::kWave) void wave_probe_kernel(waveprobe::Args a) {
  waveprobe::probe_lane<W>(a, pinkhip::block_id());
}

struct DeviceArrays {
  void *ptr[16] = {};
  int n = 0;
  ~DeviceArrays() {
    for (int i = 0; i < n; ++i) (void)hipFree(ptr[i]);
  }
  // a device copy of `bytes` bytes of host memory (src == nullptr: zero-filled)
  void *make(const void *src, size_t bytes, hipError_t &err) {
    void *p = nullptr;
    if (err != hipSuccess) return nullptr;
    err = hipMalloc(&p, bytes ? bytes : 8);
    if (err != hipSuccess) return nullptr;
    ptr[n++] = p;
    err = src ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipMemset(p, 0, bytes);
    return p;
  }
};

}  // namespace

extern "C" {

const char *wave_probe_last_error() { return g_error; }

int wave_probe_slots_d(int W) { return waveprobe::slots_d(W); }
int wave_probe_slots_i() { return waveprobe::kSlotsI; }

// Host arrays in, host arrays out: `sets` input sets of 64 lanes each, one wavefront per set.
// out_d: [sets][wave_probe_slots_d(W)][64] doubles, out_i: [sets][wave_probe_slots_i()][64] ints.
int wave_probe_run(int W, int sets, const double *v, const double *x, const double *acc, const double *key, const int *pred,
                   const int *gsrc, const int *isrc, const int *lsrc, const int *gint, const int *ival, const int *on,
                   double *out_d, int *out_i) {
  if ((W != 8 && W != 16 && W != 32 && W != 64) || sets < 1 || sets > 4096) {
    std::snprintf(g_error, sizeof g_error, "wave_probe_run: W = %d, sets = %d", W, sets);
    return -1;
  }
  const size_t n = static_cast<size_t>(sets) * pinkhip::kWave;
  const size_t nd = n * waveprobe::slots_d(W) * sizeof(double), ni = n * waveprobe::kSlotsI * sizeof(int);
  hipError_t err = hipSuccess;
  DeviceArrays d;
  waveprobe::Args a;
  a.v = static_cast<const double *>(d.make(v, n * 8, err));
  a.x = static_cast<const double *>(d.make(x, n * 8, err));
  a.acc = static_cast<const double *>(d.make(acc, n * 8, err));
  a.key = static_cast<const double *>(d.make(key, n * 8, err));
  a.pred = static_cast<const int *>(d.make(pred, n * 4, err));
  a.gsrc = static_cast<const int *>(d.make(gsrc, n * 4, err));
  a.isrc = static_cast<const int *>(d.make(isrc, n * 4, err));
  a.lsrc = static_cast<const int *>(d.make(lsrc, n * 4, err));
  a.gint = static_cast<const int *>(d.make(gint, n * 4, err));
  a.ival = static_cast<const int *>(d.make(ival, n * 4, err));
  a.on = static_cast<const int *>(d.make(on, n * 4, err));
  a.out_d = static_cast<double *>(d.make(nullptr, nd, err));
  a.out_i = static_cast<int *>(d.make(nullptr, ni, err));
  if (err == hipSuccess) {
    const dim3 grid(sets), block(pinkhip::kWave);
    switch (W) {
      case 8: wave_probe_kernel<8><<<grid, block>>>(a); break;
      case 16: wave_probe_kernel<16><<<grid, block>>>(a); break;
      case 32: wave_probe_kernel<32><<<grid, block>>>(a); break;
      default: wave_probe_kernel<64><<<grid, block>>>(a); break;
    }
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out_d, a.out_d, nd, hipMemcpyDeviceToHost);
  if (err == hipSuccess) err = hipMemcpy(out_i, a.out_i, ni, hipMemcpyDeviceToHost);
  if (err != hipSuccess) {
    std::snprintf(g_error, sizeof g_error, "wave_probe_run: %s", hipGetErrorString(err));
    return static_cast<int>(err);
  }
  return 0;
}

}  // extern "C"

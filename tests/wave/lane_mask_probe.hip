// The lane-mask primitives of pink_amd/csrc/wave.h on the device's own code path -- TEST CODE ONLY: built by
// __graft_entry__.build() into tests/wave/liblanemaskprobe.so (its own library: libpinkhip's objects and exported names do
// not change), loaded by tests/test_lane_mask_primitives.py.  The kernel body is lane_mask_probe_kernel.h, shared with the
// CPU emulator.
#include "../../pink_amd/csrc/wave.h"
// clang-format off
#include "lane_mask_probe_kernel.h"
// clang-format on

#include <cstdio>

namespace {

char g_error[256] = "";

template <int W>
__global__ __launch_bounds__(pinkhip::kWave) void lane_mask_probe_kernel(lanemaskprobe::Args a) {
  lanemaskprobe::probe_lane<W>(a, pinkhip::block_id());
}

struct DeviceArrays {
  void *ptr[8] = {};
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

const char *lane_mask_probe_last_error() { return g_error; }

int lane_mask_probe_slots(int W) { return lanemaskprobe::slots(W); }

// Host arrays in, host array out: `sets` input sets, one wavefront per set.  mask_lo, mask_hi, bits, lane: [sets];
// pred, ival, keybits: [sets][64]; out: [sets][lane_mask_probe_slots(W)][64] ints.
int lane_mask_probe_run(int W, int sets, const int *mask_lo, const int *mask_hi, const int *bits, const int *lane, const int *pred,
                        const int *ival, const int *keybits, int *out) {
  if ((W != 16 && W != 32 && W != 64) || sets < 1 || sets > 4096) {
    std::snprintf(g_error, sizeof g_error, "lane_mask_probe_run: W = %d, sets = %d", W, sets);
    return -1;
  }
  const size_t n = static_cast<size_t>(sets) * pinkhip::kWave;
  const size_t no = n * lanemaskprobe::slots(W) * sizeof(int);
  hipError_t err = hipSuccess;
  DeviceArrays d;
  lanemaskprobe::Args a;
  a.mask_lo = static_cast<const int *>(d.make(mask_lo, sets * 4, err));
  a.mask_hi = static_cast<const int *>(d.make(mask_hi, sets * 4, err));
  a.bits = static_cast<const int *>(d.make(bits, sets * 4, err));
  a.lane = static_cast<const int *>(d.make(lane, sets * 4, err));
  a.pred = static_cast<const int *>(d.make(pred, n * 4, err));
  a.ival = static_cast<const int *>(d.make(ival, n * 4, err));
  a.keybits = static_cast<const int *>(d.make(keybits, n * 4, err));
  a.out = static_cast<int *>(d.make(nullptr, no, err));
  if (err == hipSuccess) {
    const dim3 grid(sets), block(pinkhip::kWave);
    switch (W) {
      case 16: lane_mask_probe_kernel<16><<<grid, block>>>(a); break;
      case 32: lane_mask_probe_kernel<32><<<grid, block>>>(a); break;
      default: lane_mask_probe_kernel<64><<<grid, block>>>(a); break;
    }
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy(out, a.out, no, hipMemcpyDeviceToHost);
  if (err != hipSuccess) {
    std::snprintf(g_error, sizeof g_error, "lane_mask_probe_run: %s", hipGetErrorString(err));
    return static_cast<int>(err);
  }
  return 0;
}

}  // extern "C"

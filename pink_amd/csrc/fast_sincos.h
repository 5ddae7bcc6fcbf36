// fast_sincos: the one piece of wave.h's arithmetic that needs nothing from the GPU (rint and fma only), in a
// header of its own so that the CPU wave emulator (emu/wave_emu.h) executes the very same reduction and
// polynomials as the device.  Include it behind <hip/hip_runtime.h> (device) or behind the emulator's definitions
// of __device__ / __forceinline__ and <cmath>.
#pragma once

namespace pinkhip {

// sin and cos of a joint angle: Cody-Waite reduction by pi/2 in three FMAs + the fdlibm minimax kernels on
// [-pi/4, pi/4].  pi/2 = c1 + c2 + c3 to 5.6e-50: the first FMA is exact (|k| < 2^16, the difference has fewer than
// 53 bits), so the reduced argument is off by half an ulp of ITSELF plus |k| 5.6e-50 -- also for the doubles that
// lie closest to a multiple of pi/2 (below 1e5 the closest is 45.553093477052 = 29 pi/2 - 6.2e-19).  With two terms
// the reduction was off by |k| 1.5e-33 ABSOLUTE, which at those doubles is up to 1800 ulp of the sine
// (tests/test_kinematics_exact.py measures against 50-digit values: < 2 ulp for |t| < 1e5 rad, the argument's half ulp
// plus the kernels' < 1 ulp).  The libm versions carry a Payne-Hanek path for huge arguments that costs
// private-memory scratch and registers in every kernel that calls them.
__device__ __forceinline__ void fast_sincos(double t, double &sn, double &cs) {
  const double k = rint(t * 0.63661977236758134308);  // 2 / pi
  double r = fma(-k, 1.5707963267948966, t);
  r = fma(-k, 6.123233995736766e-17, r);
  r = fma(-k, -1.4973849048591698e-33, r);
  const double z = r * r;
  const double ps = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                               2.75573137070700676789e-06), -1.98412698298579493134e-04),
                               8.33333333332248946124e-03), -1.66666666666666324348e-01);
  const double pc = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                               -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                               -1.38888888888741095749e-03), 4.16666666666666019037e-02);
  const double s0 = fma(r * z, ps, r);
  const double c0 = fma(z * z, pc, fma(-0.5, z, 1.0));
  const int q = static_cast<int>(k) & 3;
  const double s1 = (q & 1) ? c0 : s0, c1 = (q & 1) ? s0 : c0;
  sn = (q & 2) ? -s1 : s1;
  cs = ((q + 1) & 2) ? -c1 : c1;
}

}  // namespace pinkhip

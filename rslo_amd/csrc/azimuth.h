// The reproducible azimuth of a return (csrc/deskew.hip, csrc/carve.hip; host twin: rslo_amd/deskew.py
// sweep_fraction_ref): a fixed arctangent polynomial instead of libm makes the turn fraction the same bits on the device
// and in numpy.
//
// Like se3.h this header carries no `#pragma clang fp contract`: its functions take the contraction state of the file
// that includes them, and both includers place the include AFTER their `fp contract(off)`.
#pragma once

#define AZ_HALF_PI 1.5707963267948966
#define AZ_PI 3.141592653589793
#define AZ_TWO_PI 6.283185307179586

// Abramowitz & Stegun 4.4.49 on [0, 1]
__device__ __forceinline__ double az_atan(double r) {
  const double z = r * r;
  double p = 0.0028662257;
  p = -0.0161657367 + z * p;
  p = 0.0429096138 + z * p;
  p = -0.0752896400 + z * p;
  p = 0.1065626393 + z * p;
  p = -0.1420889944 + z * p;
  p = 0.1999355085 + z * p;
  p = -0.3333314528 + z * p;
  p = 1.0 + z * p;
  return r * p;
}

// the sweep fraction of a return at (x, y), neither both zero: the azimuth in turns from az_start_turn, in [0, 1]
__device__ __forceinline__ double az_fraction(double x, double y, double az_start_turn, int az_clockwise) {
  const double ax = fabs(x), ay = fabs(y);
  const double lo = ax < ay ? ax : ay, hi = ax < ay ? ay : ax;
  double phi = az_atan(lo / hi);
  if (ay > ax) phi = AZ_HALF_PI - phi;
  if (x < 0.0) phi = AZ_PI - phi;
  if (y < 0.0) phi = -phi;
  double f = phi / AZ_TWO_PI - az_start_turn;
  if (az_clockwise) f = -f;
  return f - floor(f);
}

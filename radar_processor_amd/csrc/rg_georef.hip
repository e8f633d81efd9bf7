// Georeferencing (include/radargrid_hip.h, rg_georef): a radar's gates from its own azimuthal-equidistant plane into the
// plane of a shared grid, and the longitude / latitude of a grid's nodes.  Spherical AEQD, float64 throughout, one element
// per thread, coalesced loads and stores, no LDS.  The translation unit is built with FP contraction off like every other:
// the steps below are NumPy's, in the order the header writes them.
#include <math.h>

#include "rg_common.hpp"

namespace {

constexpr double kRadToDeg = 180.0 / 3.14159265358979323846;
constexpr long kPerLaunch = 1L << 31;      // a dispatch holds at most 2^32 - 1 work-items: larger arrays take several

// plane (x, y) about the `from` centre -> (lon, lat) in radians; rho != 0
__device__ __forceinline__ void aeqd_inverse(const rg_georef& g, double x, double y, double rho, double* lon, double* lat) {
  const double c = rho / g.radius;
  double sc, cc;
  sincos(c, &sc, &cc);
  const double sin_lat = cc * g.sin_lat_from + y * sc * g.cos_lat_from / rho;
  *lat = asin(fmin(fmax(sin_lat, -1.0), 1.0));       // rounding may leave |sin_lat| a last bit above 1 at a pole
  *lon = g.lon_from + atan2(x * sc, rho * g.cos_lat_from * cc - y * g.sin_lat_from * sc);
}

// (lon, lat) in radians -> plane (X, Y) about the `to` centre.  The angular distance comes from atan2(s, q): acos(q)
// would lose half the digits near the centre.
__device__ __forceinline__ void aeqd_forward(const rg_georef& g, double lon, double lat, double* X, double* Y) {
  double sp, cp, sd, cd;
  sincos(lat, &sp, &cp);
  sincos(lon - g.lon_to, &sd, &cd);
  const double a = cp * sd;
  const double b = g.cos_lat_to * sp - g.sin_lat_to * cp * cd;
  const double q = g.sin_lat_to * sp + g.cos_lat_to * cp * cd;
  const double s = hypot(a, b);
  const double k = s == 0.0 ? 1.0 : atan2(s, q) / s;
  *X = g.radius * k * a;
  *Y = g.radius * k * b;
}

// x / y may BE x_out / y_out (in place): a thread reads its own gate before it writes it, and no other thread touches it.
// Hence no __restrict__ on the four arrays.
__global__ __launch_bounds__(rg::kBlock) void gates_to_frame_kernel(const float* x, const float* y, long n, rg_georef g,
                                                                    float* x_out, float* y_out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float xf = x[i], yf = y[i];
  if (g.same_centre) {           // a radar at the grid origin stays what a single-radar build sees, bit for bit
    x_out[i] = xf;
    y_out[i] = yf;
    return;
  }
  float xo = __builtin_nanf(""), yo = xo;
  if (isfinite(xf) && isfinite(yf)) {
    const double xd = (double)xf, yd = (double)yf;
    const double rho = hypot(xd, yd);
    xo = yo = 0.0f;              // rho == 0: the antenna itself, (ox, oy) - (ox, oy)
    if (rho != 0.0) {
      double lon, lat, X, Y;
      aeqd_inverse(g, xd, yd, rho, &lon, &lat);
      aeqd_forward(g, lon, lat, &X, &Y);
      xo = (float)(X - g.ox);
      yo = (float)(Y - g.oy);
    }
  }
  x_out[i] = xo;
  y_out[i] = yo;
}

__global__ __launch_bounds__(rg::kBlock) void frame_to_lonlat_kernel(const float* __restrict__ xc, const float* __restrict__ yc,
                                                                     long first, long n, int nx, rg_georef g,
                                                                     double* __restrict__ lon_deg, double* __restrict__ lat_deg) {
  const long i = first + (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long iy = i / nx;
  const float xf = xc[i - iy * nx], yf = yc[iy];
  double lon = __builtin_nan(""), lat = lon;
  if (isfinite(xf) && isfinite(yf)) {
    const double xd = (double)xf, yd = (double)yf;
    const double rho = hypot(xd, yd);
    lon = g.lon_from;
    lat = g.lat_from;
    if (rho != 0.0) aeqd_inverse(g, xd, yd, rho, &lon, &lat);
    lon *= kRadToDeg;
    lon -= 360.0 * floor((lon + 180.0) / 360.0);     // into [-180, 180) ...
    if (lon >= 180.0) lon -= 360.0;                  // ... also where the subtraction rounded up to 180
    lat *= kRadToDeg;
  }
  lon_deg[i] = lon;
  lat_deg[i] = lat;
}

// two arrays of `bytes` bytes each share a byte without being the same array
bool overlap_apart(const void* a, const void* b, int64_t bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa != pb && pa < pb + (uintptr_t)bytes && pb < pa + (uintptr_t)bytes;
}

inline unsigned blocks_for(long n) { return (unsigned)((n + rg::kBlock - 1) / rg::kBlock); }

}  // namespace

extern "C" int rg_gates_to_frame_f32(const float* x, const float* y, int64_t n, const rg_georef* radar_to_grid,
                                     float* x_out, float* y_out, rg_stream_t stream) {
  RG_REQUIRE(x && y && radar_to_grid && x_out && y_out, RG_EINVAL, "rg_gates_to_frame_f32: null pointer");
  RG_REQUIRE(n >= 0, RG_EINVAL, "rg_gates_to_frame_f32: negative size");
  const rg_georef g = *radar_to_grid;
  RG_REQUIRE(isfinite(g.radius) && g.radius > 0.0, RG_EINVAL, "rg_gates_to_frame_f32: radius must be finite and positive");
  RG_REQUIRE(rg::georef_finite(g), RG_EINVAL, "rg_gates_to_frame_f32: a member of rg_georef is not finite");
  RG_REQUIRE(g.same_centre == 0 || g.same_centre == 1, RG_EINVAL, "rg_gates_to_frame_f32: same_centre must be 0 or 1");
  const int64_t bytes = n * (int64_t)sizeof(float);
  RG_REQUIRE(!overlap_apart(x_out, y_out, bytes) && (x_out != y_out || n == 0), RG_EINVAL,
             "rg_gates_to_frame_f32: x_out and y_out overlap");
  RG_REQUIRE(!overlap_apart(x, x_out, bytes) && !overlap_apart(x, y_out, bytes) && !overlap_apart(y, x_out, bytes) &&
                 !overlap_apart(y, y_out, bytes),
             RG_EINVAL, "rg_gates_to_frame_f32: an input overlaps an output without being the same array");
  if (n == 0) return RG_OK;
  for (int64_t first = 0; first < n; first += kPerLaunch) {
    const long m = n - first < kPerLaunch ? (long)(n - first) : kPerLaunch;
    hipLaunchKernelGGL(gates_to_frame_kernel, dim3(blocks_for(m)), dim3(rg::kBlock), 0, (hipStream_t)stream, x + first,
                       y + first, m, g, x_out + first, y_out + first);
  }
  return rg::check_launch("rg_gates_to_frame_f32");
}

extern "C" int rg_frame_to_lonlat_f64(const float* xc, const float* yc, int32_t ny, int32_t nx, const rg_georef* grid,
                                      double* lon, double* lat, rg_stream_t stream) {
  RG_REQUIRE(xc && yc && grid && lon && lat, RG_EINVAL, "rg_frame_to_lonlat_f64: null pointer");
  RG_REQUIRE(ny >= 0 && nx >= 0, RG_EINVAL, "rg_frame_to_lonlat_f64: negative size");
  const rg_georef g = *grid;
  RG_REQUIRE(isfinite(g.radius) && g.radius > 0.0, RG_EINVAL, "rg_frame_to_lonlat_f64: radius must be finite and positive");
  RG_REQUIRE(rg::georef_finite(g), RG_EINVAL, "rg_frame_to_lonlat_f64: a member of rg_georef is not finite");
  const int64_t n = (int64_t)ny * nx;
  RG_REQUIRE(!overlap_apart(lon, lat, n * (int64_t)sizeof(double)) && (lon != lat || n == 0), RG_EINVAL,
             "rg_frame_to_lonlat_f64: lon and lat overlap");
  if (n == 0) return RG_OK;
  for (int64_t first = 0; first < n; first += kPerLaunch) {
    const long m = n - first < kPerLaunch ? (long)(n - first) : kPerLaunch;
    hipLaunchKernelGGL(frame_to_lonlat_kernel, dim3(blocks_for(m)), dim3(rg::kBlock), 0, (hipStream_t)stream, xc, yc,
                       (long)first, (long)(first + m), nx, g, lon, lat);
  }
  return rg::check_launch("rg_frame_to_lonlat_f64");
}

// translation unit of k_warp_points and k_warp_map (mcba_warp_kernels.h) and the host driver of the corrected entry points:
// mcba_warp_points, mcba_undistort_maps_corrected, mcba_undistort_images_corrected
#include "mcba_debug.h"
#include "mcba_host.h"
#include "mcba_warp_driver.h"
#include "mcba_warp_kernels.h"

namespace mcba {
namespace warp {

void warp_points_launch(const WarpPointsArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  const long long blocks = (a.n + WARP_THREADS - 1) / WARP_THREADS;
  hipLaunchKernelGGL(k_warp_points, dim3(host::capped_grid(blocks, WARP_POINTS_MAX_BLOCKS)), dim3(WARP_THREADS), 0, st, a);
}

void warp_map_launch(const WarpMapArgs& a, hipStream_t st) {
  const long long per = (long long)a.H * a.W;
  if (per <= 0 || a.C <= 0) return;
  hipLaunchKernelGGL(k_warp_map, dim3((unsigned)((per + WARP_THREADS - 1) / WARP_THREADS), (unsigned)a.C), dim3(WARP_THREADS), 0, st, a);
}

}  // namespace warp
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | event-timed kernels | downloads | whole call; points or pixels written
MCBA_TIMING_GETTER(mcba_debug_warp_ms, g_warp_timing, 4)

extern "C" {

namespace {
constexpr int MAX_MAP_CAMERAS = 65535;   // blockIdx.y of k_warp_map

// what every corrected call shares beyond the scaffold: the field tables, and the camera tables of the calls that project (members:
// they go before the DeviceCall they derive from does)
struct WarpCall : DeviceCall {
  DevBuf<double> d_coef, d_size, d_cam, d_iR;
  DevBuf<int32_t> d_nd;
  DevBuf<uint8_t> d_fish;

  WarpCall() : DeviceCall(g_warp_timing) { tm.reset(); }
  warp::FieldTable fields(const warp::FieldPlan& plan) {
    upload_vector(d_coef, plan.coef, st);
    upload_vector(d_size, plan.size, st);
    return warp::FieldTable{d_coef.p, d_size.p, plan.nx, plan.ny, plan.K};
  }
  undistort::CameraTable cameras(const undistort::CameraPlan& plan) {
    upload_vector(d_cam, plan.cam, st);
    upload_vector(d_nd, plan.cam_nd, st);
    upload_vector(d_fish, plan.cam_fish, st);
    return undistort::CameraTable{d_cam.p, d_nd.p, d_fish.p};
  }
  // the arguments of k_warp_map for maps [C][height][width][2] in device memory
  warp::WarpMapArgs map_args(const undistort::CameraPlan& cams, const warp::FieldPlan& fields_plan, const std::vector<double>& iR,
                             int width, int height, float* maps) {
    warp::WarpMapArgs a{};
    a.t = cameras(cams);
    upload_vector(d_iR, iR, st);
    a.iR = d_iR.p;
    a.f = fields(fields_plan);
    a.C = fields_plan.C; a.H = height; a.W = width;
    a.maps = maps;
    return a;
  }
};

void warp_points(const mcba_field_set* f, int64_t n, const int32_t* camera_of, int32_t inverse, const double* uv, double* out,
                 uint8_t* status) {
  const char* who = "mcba_warp_points";
  WarpCall call;   // (before the buffers: see host::DeviceCall)
  warp::FieldPlan plan;
  std::string err;
  REQUIRE(n >= 0, std::string(who) + ": negative size");
  if (!warp::plan_fields(f, -1, who, plan, err)) throw Error(err);
  if (n == 0) return;                    // nothing is launched, the device is not touched
  REQUIRE(uv && out, std::string(who) + ": null argument");
  if (!undistort::check_camera_index(camera_of, n, plan.C, who, err)) throw Error(err);
  const size_t N = (size_t)n;
  DevBuf<double> d_in, d_out;
  DevBuf<int32_t> d_of;
  call.open(2);
  warp::WarpPointsArgs a{};
  a.n = n;
  a.inverse = inverse ? 1 : 0;
  a.f = call.fields(plan);
  upload_async(d_in, uv, N * 2, call.st);
  if (camera_of) upload_async(d_of, camera_of, N, call.st);
  d_out.alloc(N * 2, false);
  OutBuf<uint8_t> o_status(status, N);
  a.camera_of = camera_of ? d_of.p : nullptr;
  a.in = d_in.p; a.out = d_out.p; a.status = o_status.dev();
  call.mark(0);
  warp::warp_points_launch(a, call.st);
  call.mark(1);
  call.end_kernels("k_warp_points");
  download_async(out, d_out.p, N * 2, call.st);
  o_status.fetch(call.st);
  call.finish(n);
}

// the checks the two map-making calls share
void plan_maps(const char* who, const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P, int32_t width,
               int32_t height, undistort::CameraPlan& plan, warp::FieldPlan& fields, std::vector<double>& iR) {
  std::string err;
  if (!undistort::plan_cameras(cams, who, plan, err) || !warp::plan_fields(f, cams->C, who, fields, err) ||
      !undistort::check_image_size(cams->C, height, width, who, err) || !undistort::inverse_rectifications(plan, R, P, who, iR, err))
    throw Error(err);
  REQUIRE(cams->C <= MAX_MAP_CAMERAS, std::string(who) + ": at most 65535 cameras");
}

void maps_corrected(const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P, int32_t width, int32_t height,
                    float* maps) {
  const char* who = "mcba_undistort_maps_corrected";
  WarpCall call;   // (before the buffers: see host::DeviceCall)
  undistort::CameraPlan plan;
  warp::FieldPlan fields;
  std::vector<double> iR;
  plan_maps(who, cams, f, R, P, width, height, plan, fields, iR);
  REQUIRE(maps, std::string(who) + ": null argument");
  const size_t total = (size_t)cams->C * height * width;
  DevBuf<float> d_maps;
  call.open(2);
  d_maps.alloc(total * 2, false);
  const warp::WarpMapArgs a = call.map_args(plan, fields, iR, width, height, d_maps.p);
  call.mark(0);
  warp::warp_map_launch(a, call.st);
  call.mark(1);
  call.end_kernels("k_warp_map");
  download_async(maps, d_maps.p, total * 2, call.st);
  call.finish((int64_t)total);
}

void images_corrected(const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P, const void* src, int32_t N,
                      int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype, const int32_t* index, int32_t Hd, int32_t Wd, double border,
                      void* dst) {
  const char* who = "mcba_undistort_images_corrected";
  WarpCall call;   // (before the buffers: see host::DeviceCall)
  undistort::CameraPlan plan;
  warp::FieldPlan fields;
  std::vector<double> iR;
  std::string err;
  if (!undistort::check_image_format(channels, dtype, border, who, err) || !undistort::check_image_size(N, Hs, Ws, who, err))
    throw Error(err);
  plan_maps(who, cams, f, R, P, Wd, Hd, plan, fields, iR);
  if (N == 0) return;                    // nothing is launched, the device is not touched
  REQUIRE(src && dst && index, std::string(who) + ": null argument");
  const int M = cams->C;
  if (!undistort::check_camera_index(index, N, M, who, err)) throw Error(err);
  const size_t px = undistort::pixel_bytes(dtype) * (size_t)channels;
  const size_t src_bytes = (size_t)N * Hs * Ws * px, dst_bytes = (size_t)N * Hd * Wd * px, map_floats = (size_t)M * Hd * Wd * 2;
  DevBuf<uint8_t> d_src, d_dst;
  DevBuf<float> d_maps;              // the maps of this call: they never leave the device
  DevBuf<int32_t> d_index;
  call.open(2);
  d_maps.alloc(map_floats, false);
  const warp::WarpMapArgs m = call.map_args(plan, fields, iR, Wd, Hd, d_maps.p);
  upload_async(d_src, (const uint8_t*)src, src_bytes, call.st);
  upload_async(d_index, index, (size_t)N, call.st);
  d_dst.alloc(dst_bytes + undistort::REMAP_DST_SLACK, false);
  undistort::RemapArgs a{};
  a.maps = d_maps.p;
  a.src = d_src.p; a.dst = d_dst.p; a.index = d_index.p;
  a.N = N; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  a.border = (float)border;
  a.flat = (Wd % 4 != 0) ? 1 : 0;
  call.mark(0);
  warp::warp_map_launch(m, call.st);
  REQUIRE(undistort::remap_launch(a, channels, dtype, false, call.st), std::string(who) + ": no kernel for this image format");
  call.mark(1);
  call.end_kernels("k_warp_map + k_remap_cubic");
  download_async((uint8_t*)dst, d_dst.p, dst_bytes, call.st);
  call.finish((int64_t)N * Hd * Wd);
}
}  // namespace

int32_t mcba_warp_points(const mcba_field_set* f, int64_t n, const int32_t* camera_of_point, int32_t inverse, const double* uv,
                         double* out, uint8_t* status) {
  API_BEGIN
  warp_points(f, n, camera_of_point, inverse, uv, out, status);
  API_END
}

int32_t mcba_undistort_maps_corrected(const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P,
                                      int32_t width, int32_t height, float* maps) {
  API_BEGIN
  maps_corrected(cams, f, R, P, width, height, maps);
  API_END
}

int32_t mcba_undistort_images_corrected(const mcba_camera_set* cams, const mcba_field_set* f, const double* R, const double* P,
                                        const void* src, int32_t N, int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype,
                                        const int32_t* camera_of_image, int32_t Hd, int32_t Wd, double border, void* dst) {
  API_BEGIN
  images_corrected(cams, f, R, P, src, N, Hs, Ws, channels, dtype, camera_of_image, Hd, Wd, border, dst);
  API_END
}

}  // extern "C"

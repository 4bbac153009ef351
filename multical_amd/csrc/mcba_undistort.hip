// translation unit of k_point_ops, k_undistort_map and k_remap_cubic (mcba_undistort_kernels.h) and the host driver of the five
// undistortion entry points
#include "mcba_debug.h"
#include "mcba_host.h"
#include "mcba_undistort_driver.h"
#include "mcba_undistort_kernels.h"

namespace mcba {
namespace undistort {

namespace {
int grid_for(long long work_items, long long per_block) {
  const long long blocks = (work_items + per_block - 1) / per_block;
  return host::capped_grid(blocks, 1 << 20);
}

template <int CH, class T, bool FUSED>
void launch_remap(const RemapArgs& a, hipStream_t st) {
  long long blocks;
  if (a.flat) {
    blocks = ((long long)a.N * a.Hd * a.Wd + 3) / 4;
    blocks = (blocks + UNDISTORT_THREADS - 1) / UNDISTORT_THREADS;
  } else {
    blocks = (long long)(FUSED ? a.C : a.N) * ((a.Hd + TILE_H - 1) / TILE_H) * ((a.Wd + TILE_W - 1) / TILE_W);
  }
  if (a.flat) hipLaunchKernelGGL((k_remap_cubic<CH, T, FUSED, true>), dim3(grid_for(blocks, 1)), dim3(UNDISTORT_THREADS), 0, st, a);
  else hipLaunchKernelGGL((k_remap_cubic<CH, T, FUSED, false>), dim3(grid_for(blocks, 1)), dim3(UNDISTORT_THREADS), 0, st, a);
}

template <bool FUSED>
bool launch_remap_format(const RemapArgs& a, int channels, int dtype, hipStream_t st) {
  if (channels == 1 && dtype == PIXEL_U8) launch_remap<1, uint8_t, FUSED>(a, st);
  else if (channels == 3 && dtype == PIXEL_U8) launch_remap<3, uint8_t, FUSED>(a, st);
  else if (channels == 1 && dtype == PIXEL_F32) launch_remap<1, float, FUSED>(a, st);
  else if (channels == 3 && dtype == PIXEL_F32) launch_remap<3, float, FUSED>(a, st);
  else return false;
  return true;
}
}  // namespace

void point_ops_launch(const PointOpsArgs& a, hipStream_t st) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_point_ops, dim3(grid_for(a.n, UNDISTORT_THREADS)), dim3(UNDISTORT_THREADS), 0, st, a);
}

void undistort_map_launch(const MapArgs& a, hipStream_t st) {
  const long long total = (long long)a.C * a.H * a.W;
  if (total <= 0) return;
  hipLaunchKernelGGL(k_undistort_map, dim3(grid_for(total, UNDISTORT_THREADS)), dim3(UNDISTORT_THREADS), 0, st, a);
}

bool remap_launch(const RemapArgs& a, int channels, int dtype, bool fused, hipStream_t st) {
  if ((long long)a.N * a.Hd * a.Wd <= 0) return true;
  return fused ? launch_remap_format<true>(a, channels, dtype, st) : launch_remap_format<false>(a, channels, dtype, st);
}

}  // namespace undistort
}  // namespace mcba

using namespace mcba;
using namespace mcba::host;

// uploads | event-timed kernel | downloads | whole call; pixels written
MCBA_TIMING_GETTER(mcba_debug_undistort_ms, g_undistort_timing, 4)

extern "C" {

namespace {
// what every undistortion call shares beyond the scaffold: the camera tables on the device (members: they go before the DeviceCall
// they derive from does)
struct UndistortCall : DeviceCall {
  DevBuf<double> d_cam, d_iR;
  DevBuf<int32_t> d_nd;
  DevBuf<uint8_t> d_fish;

  UndistortCall() : DeviceCall(g_undistort_timing) { tm.reset(); }
  undistort::CameraTable cameras(const undistort::CameraPlan& plan) {
    upload_vector(d_cam, plan.cam, st);
    upload_vector(d_nd, plan.cam_nd, st);
    upload_vector(d_fish, plan.cam_fish, st);
    return undistort::CameraTable{d_cam.p, d_nd.p, d_fish.p};
  }
};

void point_ops(const char* who, bool undist, const mcba_camera_set* cams, int64_t n, const int32_t* camera_of, const double* in,
               const double* R, const double* P, double* out, uint8_t* status) {
  UndistortCall call;   // (before the buffers: see host::DeviceCall)
  undistort::CameraPlan plan;
  std::string err;
  REQUIRE(n >= 0, std::string(who) + ": negative size");
  if (!undistort::plan_cameras(cams, who, plan, err)) throw Error(err);
  if (n == 0) return;                    // nothing is launched, the device is not touched
  REQUIRE(in && out && (!undist || status), std::string(who) + ": null argument");
  if (!undistort::check_camera_index(camera_of, n, cams->C, who, err)) throw Error(err);
  const size_t N = (size_t)n, C_ = (size_t)cams->C, w = undist ? 2 : 3;
  DevBuf<double> d_in, d_out, d_R, d_P;
  DevBuf<int32_t> d_of;
  call.open(2);
  undistort::PointOpsArgs a{};
  a.undistort = undist ? 1 : 0;
  a.n = n;
  a.t = call.cameras(plan);
  upload_async(d_in, in, N * w, call.st);
  if (camera_of) upload_async(d_of, camera_of, N, call.st);
  if (R) upload_async(d_R, R, C_ * 9, call.st);
  if (P) upload_async(d_P, P, C_ * 9, call.st);
  d_out.alloc(N * 2, false);
  OutBuf<uint8_t> o_status(undist ? status : nullptr, N);
  a.camera_of = camera_of ? d_of.p : nullptr;
  a.in = d_in.p; a.R = R ? d_R.p : nullptr; a.P = P ? d_P.p : nullptr; a.out = d_out.p; a.status = o_status.dev();
  call.mark(0);
  undistort::point_ops_launch(a, call.st);
  call.mark(1);
  call.end_kernels("k_point_ops");
  download_async(out, d_out.p, N * 2, call.st);
  o_status.fetch(call.st);
  call.finish(n);
}

void undistort_maps(const mcba_camera_set* cams, const double* R, const double* P, int32_t width, int32_t height, float* maps) {
  const char* who = "mcba_undistort_maps";
  UndistortCall call;   // (before the buffers: see host::DeviceCall)
  undistort::CameraPlan plan;
  std::vector<double> iR;
  std::string err;
  if (!undistort::plan_cameras(cams, who, plan, err) || !undistort::check_image_size(cams->C, height, width, who, err) ||
      !undistort::inverse_rectifications(plan, R, P, who, iR, err))
    throw Error(err);
  REQUIRE(maps, "mcba_undistort_maps: null argument");
  const size_t total = (size_t)cams->C * height * width;
  DevBuf<float> d_maps;
  call.open(2);
  undistort::MapArgs a{};
  a.t = call.cameras(plan);
  upload_vector(call.d_iR, iR, call.st);
  a.iR = call.d_iR.p; a.C = cams->C; a.H = height; a.W = width;
  d_maps.alloc(total * 2, false);
  a.maps = d_maps.p;
  call.mark(0);
  undistort::undistort_map_launch(a, call.st);
  call.mark(1);
  call.end_kernels("k_undistort_map");
  download_async(maps, d_maps.p, total * 2, call.st);
  call.finish((int64_t)total);
}

// maps != nullptr: remap through the given maps; else the fused form through the cameras
void remap_images(const char* who, const mcba_camera_set* cams, const double* R, const double* P, const float* maps, int32_t M,
                  const void* src, int32_t N, int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype, const int32_t* index, int32_t Hd,
                  int32_t Wd, double border, void* dst) {
  const bool fused = maps == nullptr;
  UndistortCall call;   // (before the buffers: see host::DeviceCall)
  undistort::CameraPlan plan;
  std::vector<double> iR;
  std::string err;
  if (!undistort::check_image_format(channels, dtype, border, who, err) || !undistort::check_image_size(N, Hs, Ws, who, err) ||
      !undistort::check_image_size(N, Hd, Wd, who, err))
    throw Error(err);
  if (fused) {
    if (!undistort::plan_cameras(cams, who, plan, err) || !undistort::inverse_rectifications(plan, R, P, who, iR, err)) throw Error(err);
    M = cams->C;
  } else {
    REQUIRE(M > 0, std::string(who) + ": no maps");
  }
  if (N == 0) return;                    // nothing is launched, the device is not touched
  REQUIRE(src && dst && index, std::string(who) + ": null argument");
  if (!undistort::check_camera_index(index, N, M, who, err)) throw Error(err);
  const size_t px = undistort::pixel_bytes(dtype) * (size_t)channels;
  const size_t src_bytes = (size_t)N * Hs * Ws * px, dst_bytes = (size_t)N * Hd * Wd * px, map_floats = fused ? 0 : (size_t)M * Hd * Wd * 2;
  DevBuf<uint8_t> d_src, d_dst;
  DevBuf<float> d_maps;
  DevBuf<int32_t> d_index, d_by_camera;
  call.open(2);
  undistort::RemapArgs a{};
  std::vector<int32_t> by_camera;        // camera_start [M + 1] | camera_images [N]
  if (fused) {
    a.t = call.cameras(plan);
    upload_vector(call.d_iR, iR, call.st);
    a.iR = call.d_iR.p;
    a.C = M;
    undistort::images_by_camera(index, N, M, by_camera);
    upload_vector(d_by_camera, by_camera, call.st);
    a.camera_start = d_by_camera.p;
    a.camera_images = d_by_camera.p + M + 1;
  } else {
    upload_async(d_maps, maps, map_floats, call.st);
    a.maps = d_maps.p;
  }
  upload_async(d_src, (const uint8_t*)src, src_bytes, call.st);
  upload_async(d_index, index, (size_t)N, call.st);
  d_dst.alloc(dst_bytes + undistort::REMAP_DST_SLACK, false);
  a.src = d_src.p; a.dst = d_dst.p; a.index = d_index.p;
  a.N = N; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  a.border = (float)border;
  a.flat = (Wd % 4 != 0) ? 1 : 0;
  call.mark(0);
  REQUIRE(undistort::remap_launch(a, channels, dtype, fused, call.st), std::string(who) + ": no kernel for this image format");
  call.mark(1);
  call.end_kernels("k_remap_cubic");
  download_async((uint8_t*)dst, d_dst.p, dst_bytes, call.st);
  call.finish((int64_t)N * Hd * Wd);
}
}  // namespace

int32_t mcba_project_points(const mcba_camera_set* cams, int64_t n, const int32_t* camera_of_point, const double* X, double* uv) {
  API_BEGIN
  point_ops("mcba_project_points", false, cams, n, camera_of_point, X, nullptr, nullptr, uv, nullptr);
  API_END
}

int32_t mcba_undistort_points(const mcba_camera_set* cams, int64_t n, const int32_t* camera_of_point, const double* uv,
                              const double* R, const double* P, double* out, uint8_t* status) {
  API_BEGIN
  point_ops("mcba_undistort_points", true, cams, n, camera_of_point, uv, R, P, out, status);
  API_END
}

int32_t mcba_undistort_maps(const mcba_camera_set* cams, const double* R, const double* P, int32_t width, int32_t height,
                            float* maps) {
  API_BEGIN
  undistort_maps(cams, R, P, width, height, maps);
  API_END
}

int32_t mcba_remap(const void* src, int32_t N, int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype, const float* maps,
                   int32_t M, int32_t Hd, int32_t Wd, const int32_t* map_of_image, double border, void* dst) {
  API_BEGIN
  REQUIRE(maps, "mcba_remap: null argument");
  remap_images("mcba_remap", nullptr, nullptr, nullptr, maps, M, src, N, Hs, Ws, channels, dtype, map_of_image, Hd, Wd, border, dst);
  API_END
}

int32_t mcba_undistort_images(const mcba_camera_set* cams, const double* R, const double* P, const void* src, int32_t N,
                              int32_t Hs, int32_t Ws, int32_t channels, int32_t dtype, const int32_t* camera_of_image, int32_t Hd,
                              int32_t Wd, double border, void* dst) {
  API_BEGIN
  remap_images("mcba_undistort_images", cams, R, P, nullptr, 0, src, N, Hs, Ws, channels, dtype, camera_of_image, Hd, Wd, border, dst);
  API_END
}

}  // extern "C"

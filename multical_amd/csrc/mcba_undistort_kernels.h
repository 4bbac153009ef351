// mcba_undistort_kernels.h -- the kernels of mcba_undistort.h: k_point_ops, k_undistort_map and k_remap_cubic.
//
//   * k_point_ops: project or undistort, one point per lane in a grid-stride loop; the camera family is a switch per point.
//   * k_undistort_map: one destination pixel per lane, map_coordinate, one 8-byte store -- a wavefront writes 512 contiguous bytes.
//   * k_remap_cubic<CH, T, FUSED, FLAT>: the hot path.  A lane owns FOUR consecutive destination pixels and stores them as whole dwords
//     (uint8: CH dwords, float32: CH 16-byte stores) -- never a byte store.  FUSED = false reads the four coordinates from a map (two
//     16-byte loads on the row path); FUSED = true calls map_coordinate, the function k_undistort_map stores: undistort_images is
//     remap(image, undistort_maps) by construction, and the 8 bytes a pixel of map never move.  On the row path the FUSED kernel
//     walks (camera, tile) and samples EVERY image of the camera with the four coordinates it computed once: the FP64 projection
//     is paid per camera, as in the two-step route, not per image (per image it made the fused call 1.7x slower than the two-step
//     one at 16 images a camera, profiles/undistort_timing.txt).
//     Two index paths (FLAT), chosen by the launcher:
//       row path   (Wd a multiple of 4): a workgroup covers a tile of 256 pixels x 4 rows, wave w row w of it, lane l pixels 4 l .. 4 l + 3;
//                  a wavefront writes 256 contiguous pixels of one row, the four rows of a tile share source rows in L1;
//       flat path  (any other width): the images of the call are one flat run of pixels cut into groups of four; a group may straddle
//                  the end of a row or of an image, so every pixel of it finds its own (image, row, column).  The groups are still
//                  dword-aligned in the output; the last group of the call may be partial (the buffer is allocated with slack).
//     The source taps are direct loads: a tile's taps lie in a compact window of the source that L1 / L2 serve.
// No LDS, no barrier, no atomics, no cross-block waits.
#pragma once
#include <hip/hip_runtime.h>
#include "mcba_undistort.h"

namespace mcba {
namespace undistort {

struct CameraTable {
  const double* cam;          // [C][CAM_STRIDE]
  const int32_t* nd;          // [C]
  const uint8_t* fish;        // [C]
};

struct PointOpsArgs {
  int undistort;              // 0: project X [n][3] -> out [n][2]; 1: undistort uv [n][2] -> out [n][2], status [n]
  long long n;
  CameraTable t;
  const int32_t* camera_of;   // [n] or null = camera 0
  const double* in;
  const double* R;            // [C][9] or null
  const double* P;            // [C][9] or null
  double* out;
  uint8_t* status;
};

struct MapArgs {
  CameraTable t;
  const double* iR;           // [C][9]
  int C, H, W;
  float* maps;                // [C][H][W][2]
};

struct RemapArgs {
  const void* src;            // [N][Hs][Ws][CH]
  void* dst;                  // [N][Hd][Wd][CH]
  int N, Hs, Ws, Hd, Wd;
  int C;                      // cameras                    (FUSED = true)
  const int32_t* index;       // [N] map (FUSED: camera) of every image
  const int32_t* camera_start;   // [C + 1] the images of camera c are camera_images[camera_start[c] .. camera_start[c + 1])   (FUSED, row path)
  const int32_t* camera_images;  // [N] image indices, camera by camera, ascending inside a camera                               (FUSED, row path)
  const float* maps;          // [M][Hd][Wd][2]             (FUSED = false)
  CameraTable t;              //                            (FUSED = true)
  const double* iR;           // [C][9]                     (FUSED = true)
  float border;
  int flat;                   // 0: row path, 1: flat path
};

constexpr int UNDISTORT_THREADS = 256;
constexpr int TILE_W = 256, TILE_H = UNDISTORT_THREADS / 64;

__global__ __launch_bounds__(UNDISTORT_THREADS) void k_point_ops(PointOpsArgs a) {
  const long long stride = (long long)gridDim.x * UNDISTORT_THREADS;
  for (long long i = (long long)blockIdx.x * UNDISTORT_THREADS + threadIdx.x; i < a.n; i += stride) {
    const int c = a.camera_of ? a.camera_of[i] : 0;
    const double* cam = a.t.cam + (size_t)c * CAM_STRIDE;
    const int nd = a.t.nd[c];
    const bool fish = a.t.fish[c] != 0;
    double o[2];
    if (a.undistort) {
      const int st = undistort_pixel(cam, nd, fish, a.R ? a.R + 9 * (size_t)c : nullptr, a.P ? a.P + 9 * (size_t)c : nullptr,
                                     a.in[2 * i], a.in[2 * i + 1], o);
      a.status[i] = (uint8_t)st;
    } else {
      const double X[3] = {a.in[3 * i], a.in[3 * i + 1], a.in[3 * i + 2]};
      project_any(cam, nd, fish, X, o);
    }
    a.out[2 * i] = o[0];
    a.out[2 * i + 1] = o[1];
  }
}

__global__ __launch_bounds__(UNDISTORT_THREADS) void k_undistort_map(MapArgs a) {
  const long long per = (long long)a.H * a.W, total = per * a.C;
  const long long stride = (long long)gridDim.x * UNDISTORT_THREADS;
  for (long long i = (long long)blockIdx.x * UNDISTORT_THREADS + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i / per);
    const long long r = i - (long long)c * per;
    const int y = (int)(r / a.W), x = (int)(r - (long long)y * a.W);
    float2 m;
    map_coordinate(a.t.cam + (size_t)c * CAM_STRIDE, a.t.nd[c], a.t.fish[c] != 0, a.iR + 9 * (size_t)c, (double)x, (double)y, m.x, m.y);
    reinterpret_cast<float2*>(a.maps)[i] = m;
  }
}

// the coordinates of the four pixels (x0 .. x0 + 3, y) of camera c: ONE copy of the FP64 projection in a rolled loop, the results
// picked into registers by constant-index selects (no dynamic register indexing, no scratch) -- four inlined copies cost the kernel
// 256 VGPRs and one wave a SIMD
__device__ __forceinline__ void quad_coordinates(const RemapArgs& a, int c, int x0, int y, float* mx, float* my) {
  const double* cam = a.t.cam + (size_t)c * CAM_STRIDE;
  const int nd = a.t.nd[c];
  const bool fish = a.t.fish[c] != 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) mx[j] = my[j] = 0.0f;
#pragma nounroll
  for (int i = 0; i < 4; ++i) {
    float tx, ty;
    map_coordinate(cam, nd, fish, a.iR + 9 * (size_t)c, (double)(x0 + i), (double)y, tx, ty);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mx[j] = (i == j) ? tx : mx[j];
      my[j] = (i == j) ? ty : my[j];
    }
  }
}

// samples the four pixels (image img[i], coordinate mx[i], my[i]; live[i] == false: a pixel past the end of the call) and stores
// them as the CH dwords / 16-byte words that start at flat pixel index p0 (a multiple of 4)
template <int CH, class T>
__device__ __forceinline__ void sample_store(const RemapArgs& a, long long p0, const int* img, const bool* live, const float* mx,
                                             const float* my) {
  float v[4 * CH];
  const size_t image_elems = (size_t)a.Hs * a.Ws * CH;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (live[i]) {
      remap_pixel<CH, T>(static_cast<const T*>(a.src) + (size_t)img[i] * image_elems, a.Hs, a.Ws, mx[i], my[i], a.border, v + i * CH);
    } else {
#pragma unroll
      for (int c = 0; c < CH; ++c) v[i * CH + c] = 0.0f;
    }
  }
  if constexpr (sizeof(T) == 1) {
    uint32_t* out = static_cast<uint32_t*>(a.dst) + (size_t)p0 / 4 * CH;
#pragma unroll
    for (int d = 0; d < CH; ++d)
      out[d] = (uint32_t)saturate_u8(v[4 * d]) | (uint32_t)saturate_u8(v[4 * d + 1]) << 8 | (uint32_t)saturate_u8(v[4 * d + 2]) << 16 |
               (uint32_t)saturate_u8(v[4 * d + 3]) << 24;
  } else {
    float4* out = static_cast<float4*>(a.dst) + (size_t)p0 / 4 * CH;
#pragma unroll
    for (int d = 0; d < CH; ++d) out[d] = make_float4(v[4 * d], v[4 * d + 1], v[4 * d + 2], v[4 * d + 3]);
  }
}

// flat path: the four pixels that start at flat pixel index p0 = (image n, row y, column x0), each with its own image and row
template <int CH, class T, bool FUSED>
__device__ __forceinline__ void remap_quad_flat(const RemapArgs& a, long long p0, int n, int y, int x0) {
  const long long per = (long long)a.Hd * a.Wd, total = per * a.N;
  float mx[4], my[4];
  int img[4];
  bool live[4];
  int ni = n, yi = y, xi = x0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    live[i] = p0 + i < total;
    img[i] = live[i] ? ni : 0;
    mx[i] = my[i] = 0.0f;
    if (live[i]) {
      const int m = a.index[ni];
      if constexpr (FUSED) {
        map_coordinate(a.t.cam + (size_t)m * CAM_STRIDE, a.t.nd[m], a.t.fish[m] != 0, a.iR + 9 * (size_t)m, (double)xi, (double)yi,
                       mx[i], my[i]);
      } else {
        const float2 c = reinterpret_cast<const float2*>(a.maps)[(size_t)m * per + (size_t)yi * a.Wd + xi];
        mx[i] = c.x;
        my[i] = c.y;
      }
    }
    if (++xi == a.Wd) {            // the next pixel opens a row (and perhaps an image)
      xi = 0;
      if (++yi == a.Hd) { yi = 0; ++ni; }
    }
  }
  sample_store<CH, T>(a, p0, img, live, mx, my);
}

template <int CH, class T, bool FUSED, bool FLAT>
__global__ __launch_bounds__(UNDISTORT_THREADS) void k_remap_cubic(RemapArgs a) {
  const long long per = (long long)a.Hd * a.Wd;
  if constexpr (!FLAT) {
    // row path.  The slices of the tile loop are the images (FUSED: the cameras, whose coordinates serve all their images)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tiles_x = (a.Wd + TILE_W - 1) / TILE_W, tiles_y = (a.Hd + TILE_H - 1) / TILE_H;
    const long long n_tiles = (long long)(FUSED ? a.C : a.N) * tiles_y * tiles_x;
    const bool live[4] = {true, true, true, true};
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
      const int tx = (int)(t % tiles_x);
      const long long r = t / tiles_x;
      const int ty = (int)(r % tiles_y), slice = (int)(r / tiles_y);
      const int y = ty * TILE_H + wave, x0 = tx * TILE_W + 4 * lane;
      if (y >= a.Hd || x0 >= a.Wd) continue;            // (Wd is a multiple of 4: a group is inside the row or outside)
      const long long in_image = (long long)y * a.Wd + x0;
      float mx[4], my[4];
      if constexpr (FUSED) {
        const int first = a.camera_start[slice], last = a.camera_start[slice + 1];
        if (first == last) continue;                    // (a camera without images)
        quad_coordinates(a, slice, x0, y, mx, my);
#pragma nounroll
        for (int k = first; k < last; ++k) {
          const int n = a.camera_images[k];
          const int img[4] = {n, n, n, n};
          // (the coordinates are loop-invariant, and so are the weights and the 64 tap offsets behind them: hoisted, they cost
          //  the kernel 256 VGPRs and one wave a SIMD.  Opaque to the optimiser, the body is that of the map-fed kernel.)
#pragma unroll
          for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(mx[i]), "+v"(my[i]));
          sample_store<CH, T>(a, (long long)n * per + in_image, img, live, mx, my);
        }
      } else {
        const int m = a.index[slice];
        const float4* q = reinterpret_cast<const float4*>(a.maps + ((size_t)m * per + (size_t)in_image) * 2);   // 32-byte aligned
        const float4 c0 = q[0], c1 = q[1];
        mx[0] = c0.x; my[0] = c0.y; mx[1] = c0.z; my[1] = c0.w;
        mx[2] = c1.x; my[2] = c1.y; mx[3] = c1.z; my[3] = c1.w;
        const int img[4] = {slice, slice, slice, slice};
        sample_store<CH, T>(a, (long long)slice * per + in_image, img, live, mx, my);
      }
    }
  } else {
    const long long groups = (per * a.N + 3) / 4;
    const long long stride = (long long)gridDim.x * UNDISTORT_THREADS;
    for (long long g = (long long)blockIdx.x * UNDISTORT_THREADS + threadIdx.x; g < groups; g += stride) {
      const long long p0 = 4 * g;
      const int n = (int)(p0 / per);
      const long long r = p0 - (long long)n * per;
      const int y = (int)(r / a.Wd), x0 = (int)(r - (long long)y * a.Wd);
      remap_quad_flat<CH, T, FUSED>(a, p0, n, y, x0);
    }
  }
}

// bytes the launcher may write past the last pixel of dst (a partial last group of the flat path)
constexpr size_t REMAP_DST_SLACK = 64;

void point_ops_launch(const PointOpsArgs& a, hipStream_t st);                                       // mcba_undistort.hip
void undistort_map_launch(const MapArgs& a, hipStream_t st);
bool remap_launch(const RemapArgs& a, int channels, int dtype, bool fused, hipStream_t st);        // false: no such instantiation

}  // namespace undistort
}  // namespace mcba

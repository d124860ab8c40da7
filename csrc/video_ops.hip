// Video-side and head kernels for the R(2+1)D pipeline on CDNA4.
//
//  * rnb_clipgen_u8     synthetic "decoder surface": 8-frame clips of
//                        HxWx3 uint8 pixels, deterministic per (video, frame)
//                        -- stands in for the rocDecode/VCN output (SURVEY.md
//                        K30; no decoder or dataset on the target machines).
//  * rnb_preprocess      uint8 NFHWC3 -> normalised bf16 NDHWC8 (channels 3..7
//                        zero), the fused form of the reference's
//                        .float().permute() + slot copy.
//  * rnb_nv12_to_clip    decoder surfaces (NV12) -> scaled, colour-converted,
//                        normalised clips in the slot layout.
//  * rnb_yuv_to_clip_boxes
//                        the same from uploaded file spans (planar 4:2:0 /
//                        4:2:2 / 4:4:4 of .y4m files and JPEG surfaces, raw
//                        NV12), bilinear or with the antialiased triangle filter
//                        (separable through LDS), with a crop box per row, so
//                        that several views of one clip read one uploaded span.
//  * rnb_stem_pack       NDHWC8 -> zero-bordered pixel-pair-packed layout of
//                        the stem conv (ops/conv.StemConv).
//  * rnb_preprocess_packed  rnb_preprocess + rnb_stem_pack in one pass: uint8
//                        frames straight to the stem's packed input.
//  * rnb_head            AdaptiveAvgPool3d(1) + Linear(512 -> classes): a
//                        pooling kernel (one thread per clip x channel pair)
//                        and a linear kernel (16 clips x 64 classes per block)
//                        (SURVEY.md K28).
//  * rnb_video_reduce    per-video sum of clip logits + argmax, the GPU form
//                        of R2P1DAggregator's reduction.
#include <hip/hip_runtime.h>
#include <stdint.h>

static __device__ __forceinline__ uint32_t pixel_hash(uint32_t vid, uint32_t frame,
                                                      uint32_t pix, uint32_t c) {
  uint32_t h = vid * 0x9E3779B1u + frame * 0x85EBCA77u + pix * 0xC2B2AE3Du + c * 0x27D4EB2Fu;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return h >> 24;
}

// out[clip][f][y][x][c]; one thread = 16 consecutive pixels (48 bytes) of one
// frame (H*W is a multiple of 16 for the 112x112 clips; a tail is handled).
__global__ void clipgen_u8_kernel(uint8_t* __restrict__ out, const int* __restrict__ vids,
                                  const int* __restrict__ starts, int nclips, int F, int H,
                                  int W) {
  const long long hw = (long long)H * W;
  const long long total_px = hw * F * nclips;
  const long long px0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (px0 >= total_px) return;
  const long long frame = px0 / hw;                  // clip * F + f
  const int clip = (int)(frame / F);
  const uint32_t vid = (uint32_t)vids[clip];
  const uint32_t fr = (uint32_t)(starts[clip] + (int)(frame - (long long)clip * F));
  const uint32_t pix0 = (uint32_t)(px0 - frame * hw);
  const int n = (int)min(16LL, min(total_px - px0, hw - (long long)pix0));
  uint32_t words[12];
#pragma unroll
  for (int w = 0; w < 12; ++w) words[w] = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int b = i * 3 + c;
      const uint32_t v = i < n ? pixel_hash(vid, fr, pix0 + i, c) : 0u;
      words[b >> 2] |= v << (8 * (b & 3));
    }
  }
  uint8_t* dst = out + px0 * 3;
  if (n == 16) {
    uint4* d4 = (uint4*)dst;                         // 48 * t bytes: 16-B aligned
    d4[0] = make_uint4(words[0], words[1], words[2], words[3]);
    d4[1] = make_uint4(words[4], words[5], words[6], words[7]);
    d4[2] = make_uint4(words[8], words[9], words[10], words[11]);
  } else {
    for (int b = 0; b < n * 3; ++b) dst[b] = (uint8_t)(words[b >> 2] >> (8 * (b & 3)));
  }
}

// Same generator for ONE video whose clip start frames travel in the kernel
// arguments (no metadata upload, no host synchronisation: the loader stage
// issues it per video; rnb_amd/models/r2p1d/decoder.py).
#define CLIPGEN_MAX_CLIPS 32
// step_p / step_q: frame f of a clip is source frame start + (f * step_p) /
// step_q (sampler.clip_frames); the launcher keeps F * step_p inside an int.
struct ClipgenArgs {
  int vid, nclips;
  int step_p, step_q;
  int starts[CLIPGEN_MAX_CLIPS];
};

__global__ void clipgen_video_kernel(uint8_t* __restrict__ out, ClipgenArgs a, int F, int H,
                                     int W) {
  const long long hw = (long long)H * W;
  const long long total_px = hw * F * a.nclips;
  const long long px0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (px0 >= total_px) return;
  const long long frame = px0 / hw;
  const int clip = (int)(frame / F);
  const uint32_t vid = (uint32_t)a.vid;
  const int f = (int)(frame - (long long)clip * F);
  const uint32_t fr = (uint32_t)(a.starts[clip] + (f * a.step_p) / a.step_q);
  const uint32_t pix0 = (uint32_t)(px0 - frame * hw);
  const int n = (int)min(16LL, min(total_px - px0, hw - (long long)pix0));
  uint32_t words[12];
#pragma unroll
  for (int w = 0; w < 12; ++w) words[w] = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int b = i * 3 + c;
      const uint32_t v = i < n ? pixel_hash(vid, fr, pix0 + i, c) : 0u;
      words[b >> 2] |= v << (8 * (b & 3));
    }
  }
  uint8_t* dst = out + px0 * 3;
  if (n == 16) {
    uint4* d4 = (uint4*)dst;
    d4[0] = make_uint4(words[0], words[1], words[2], words[3]);
    d4[1] = make_uint4(words[4], words[5], words[6], words[7]);
    d4[2] = make_uint4(words[8], words[9], words[10], words[11]);
  } else {
    for (int b = 0; b < n * 3; ++b) dst[b] = (uint8_t)(words[b >> 2] >> (8 * (b & 3)));
  }
}

// ---------------------------------------------------------------------------
// NV12 decoder surfaces -> normalised clips: the per-frame work NVVL's
// RnBLoader does after NVDEC (colour conversion + scaling to 112x112;
// reference models/r2p1d/model.py:123-125, README.md:42-110).
//
//  * nv12gen_video_kernel   synthetic decoder output: NV12 frames (Y plane of
//                           H rows, then an interleaved UV plane of H/2 rows,
//                           W bytes per row) at the source resolution, e.g.
//                           Kinetics' 340x256; stands in for the VCN surface.
//  * nv12_clip_kernel       bilinear scale (align_corners = false, from a crop
//                           box of the source frame) of Y and of the half-
//                           resolution U/V planes, BT.601 video-range YUV ->
//                           RGB, clamp to [0, 255], Kinetics normalisation,
//                           written straight into the stage's NDHWC layout
//                           (fp32 4 channels or bf16 8 channels per pixel).
// ---------------------------------------------------------------------------
template <bool FROM_ARRAYS>
__global__ void nv12gen_kernel(uint8_t* __restrict__ out, ClipgenArgs a,
                               const int* __restrict__ vids, const int* __restrict__ starts,
                               int F, int H, int W) {
  // one thread = 16 bytes of one frame's NV12 image (H*W*3/2 bytes per frame)
  const long long fbytes = (long long)H * W * 3 / 2;
  const long long total = fbytes * F * a.nclips;
  const long long b0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 16;
  if (b0 >= total) return;
  const long long frame = b0 / fbytes;
  const int clip = (int)(frame / F);
  const int start = FROM_ARRAYS ? starts[clip] : a.starts[clip];
  const uint32_t vid = (uint32_t)(FROM_ARRAYS ? vids[clip] : a.vid);
  const int f = (int)(frame - (long long)clip * F);
  // the device-array form has no step: its clips are consecutive frames
  const uint32_t fr = (uint32_t)(start + (FROM_ARRAYS ? f : (f * a.step_p) / a.step_q));
  const long long off0 = b0 - frame * fbytes;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long off = off0 + i;
    uint32_t v = 0;
    if (off < fbytes) {
      if (off < (long long)H * W) {
        v = pixel_hash(vid, fr, (uint32_t)off, 0u);
      } else {
        const long long c = off - (long long)H * W;     // UV plane byte
        v = pixel_hash(vid, fr, (uint32_t)(c >> 1), 1u + (uint32_t)(c & 1));
        v = 64u + (v >> 1);                              // keep chroma near neutral
      }
    }
    w[i >> 2] |= v << (8 * (i & 3));
  }
  uint8_t* dst = out + b0;
  if (off0 + 16 <= fbytes && ((uintptr_t)dst & 15u) == 0) {
    *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (int i = 0; i < 16 && off0 + i < fbytes; ++i) dst[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

struct NormParams {
  float scale[3];   // 1 / (255 * std)
  float shift[3];   // -mean / std
};

static NormParams norm_params(const float* mean, const float* stdv) {
  NormParams n;
  for (int c = 0; c < 3; ++c) {
    n.scale[c] = 1.0f / (255.0f * stdv[c]);
    n.shift[c] = -mean[c] / stdv[c];
  }
  return n;
}

struct ClipGeometry {
  int src_w, src_h, out_w, out_h;
};

struct Nv12ClipArgs {
  ClipGeometry g;
  float crop_x, crop_y, crop_w, crop_h;   // source box scaled to the output
  NormParams norm;
  int bf16;                               // 0: fp32 NDHWC4, 1: bf16 NDHWC8
};

static __device__ __forceinline__ uint32_t f2bf_bits(float f) {
  // round-to-nearest-even (inputs are finite)
  uint32_t u = __float_as_uint(f);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// What the clip kernels do with a resampled pixel: yv and the chroma samples
// less 128 -> RGB (JFIF: full-range JFIF YCbCr, else video-range BT.601), clamp
// to [0, 255], normalise, store as output pixel i (bf16 NDHWC8 or fp32 NDHWC4).
// n by value: a reference into the kernel's argument struct makes the compiler
// recompute the antialias kernel's per-plane set-up for the chroma planes.
template <bool JFIF>
static __device__ __forceinline__ void clip_store(float yv, float u, float v,
                                                  const NormParams n, int bf16, void* out,
                                                  long long i) {
  const float yy = JFIF ? yv : 1.164f * (yv - 16.f);
  float r = yy + (JFIF ? 1.402f : 1.596f) * v;
  float g = yy - (JFIF ? 0.344136f : 0.392f) * u - (JFIF ? 0.714136f : 0.813f) * v;
  float b = yy + (JFIF ? 1.772f : 2.017f) * u;
  r = fminf(fmaxf(r, 0.f), 255.f) * n.scale[0] + n.shift[0];
  g = fminf(fmaxf(g, 0.f), 255.f) * n.scale[1] + n.shift[1];
  b = fminf(fmaxf(b, 0.f), 255.f) * n.scale[2] + n.shift[2];
  if (bf16) {
    uint16_t* o = (uint16_t*)out + i * 8;
    *(uint4*)o = make_uint4(f2bf_bits(r) | (f2bf_bits(g) << 16), f2bf_bits(b), 0u, 0u);
  } else {
    *(float4*)((float*)out + i * 4) = make_float4(r, g, b, 0.f);
  }
}

static __device__ __forceinline__ float nv12_sample(const uint8_t* __restrict__ plane, int w,
                                                    int h, int stride, int comps, int comp,
                                                    float sx, float sy) {
  // bilinear with edge clamping, align_corners = false mapping done by caller
  sx = fminf(fmaxf(sx, 0.f), (float)(w - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(h - 1));
  const int x0 = (int)sx, y0 = (int)sy;
  const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
  const float fx = sx - (float)x0, fy = sy - (float)y0;
  const float p00 = plane[y0 * stride + x0 * comps + comp];
  const float p01 = plane[y0 * stride + x1 * comps + comp];
  const float p10 = plane[y1 * stride + x0 * comps + comp];
  const float p11 = plane[y1 * stride + x1 * comps + comp];
  const float top = p00 + (p01 - p00) * fx;
  const float bot = p10 + (p11 - p10) * fx;
  return top + (bot - top) * fy;
}

__global__ __launch_bounds__(256) void nv12_clip_kernel(const uint8_t* __restrict__ nv12,
                                                        void* __restrict__ out, long long npix,
                                                        Nv12ClipArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const int ohw = a.g.out_w * a.g.out_h;
  const long long frame = i / ohw;
  const int p = (int)(i - frame * ohw);
  const int oy = p / a.g.out_w, ox = p - oy * a.g.out_w;
  const uint8_t* y_plane = nv12 + frame * ((long long)a.g.src_w * a.g.src_h * 3 / 2);
  const uint8_t* uv_plane = y_plane + (long long)a.g.src_w * a.g.src_h;
  // output pixel centre -> source coordinate (align_corners = false)
  const float sx = a.crop_x + ((float)ox + 0.5f) * (a.crop_w / (float)a.g.out_w) - 0.5f;
  const float sy = a.crop_y + ((float)oy + 0.5f) * (a.crop_h / (float)a.g.out_h) - 0.5f;
  const float yv = nv12_sample(y_plane, a.g.src_w, a.g.src_h, a.g.src_w, 1, 0, sx, sy);
  // chroma grid: half resolution, sample centres at 2x + 0.5
  const float cx = (sx + 0.5f) * 0.5f - 0.5f, cy = (sy + 0.5f) * 0.5f - 0.5f;
  const int cw = a.g.src_w / 2, ch = a.g.src_h / 2;
  const float u = nv12_sample(uv_plane, cw, ch, a.g.src_w, 2, 0, cx, cy) - 128.f;
  const float v = nv12_sample(uv_plane, cw, ch, a.g.src_w, 2, 1, cx, cy) - 128.f;
  clip_store<false>(yv, u, v, a.norm, a.bf16, out, i);
}

// Planar / semi-planar YUV 4:2:0 frames inside an uploaded byte buffer (file
// spans of a .y4m video, or raw NV12 dumps) -> the same normalised clips.
// Frame f of clip c starts at byte offs[c] + f * frame_stride; its Y, U and V
// samples start y_off / u_off / v_off bytes further on, with their own row
// strides, and chroma samples are c_step bytes apart (1: planar I420, 2:
// interleaved NV12 with v_off = u_off + 1). A Y4M frame is "FRAME\n" + payload,
// so none of these bases is aligned to more than a byte: every source access
// is a byte load (nv12_sample), and only the output side is vectorised. The
// launcher checked every span against the buffer length.
//
// Row c of a launch reads the frames at offs[c] through its own crop box, so
// several views of one clip share one uploaded span (rows may repeat an offset).
// Up to YUV_BOX_MAX_ROWS rows travel in the kernel arguments, offset (8 B) next
// to box (16 B, one s_load_dwordx4): 1536 B of tables, 1648 B in all, under the
// 4 KB of a dispatch packet's argument segment. 64, because a 15-clip request
// with three views is 45 rows. More rows read both tables from device memory
// (offs, boxes_dev). The row is uniform per block: scalar loads either way.
#define YUV_BOX_MAX_ROWS 64
struct __attribute__((aligned(16))) YuvBox {
  float x, y, w, h;                        // luma pixels, as Nv12ClipArgs.crop_*
};
struct YuvClipArgs {
  ClipGeometry g;
  NormParams norm;
  int bf16;                                // 0: fp32 NDHWC4, 1: bf16 NDHWC8
  int F, y_stride, u_stride, v_stride, c_step;
  long long frame_stride, y_off, u_off, v_off;
  const YuvBox* boxes_dev;                 // FROM_ARRAY: per-row boxes (else unused)
  long long offs[YUV_BOX_MAX_ROWS];        // per-row base (FROM_ARRAY: unused)
  YuvBox boxes[YUV_BOX_MAX_ROWS];          // per-row box (FROM_ARRAY: unused)
};
static_assert(sizeof(YuvClipArgs) <= 2048, "clip arguments outgrew their budget");

// JFIF: full-range JFIF YCbCr (what JPEG frames hold) instead of the video-range
// BT.601 matrix; the chroma planes of an odd-sized frame then round up.
// HS, VS: the luma sampling factors per axis, 2x2 (4:2:0), 2x1 (4:2:2) or 1x1
// (4:4:4); the chroma planes are 1x1. Chroma sample j sits at luma coordinate
// HS j + (HS - 1) / 2 (centre siting), so along an axis with factor 1 the
// chroma coordinate is the luma coordinate and the plane has the luma size.
template <int S>
static __device__ __forceinline__ int chroma_dim(int n, bool round_up) {
  return S == 2 ? (round_up ? (n + 1) / 2 : n / 2) : n;
}

// nv12_sample with the taps split from the fetch: with 1x1 factors the three
// planes share indices and weights, which are then computed once per pixel
struct BilinearTaps {
  int x0, x1, y0, y1;
  float fx, fy;
};

static __device__ __forceinline__ BilinearTaps bilinear_taps(int w, int h, float sx, float sy) {
  BilinearTaps t;
  sx = fminf(fmaxf(sx, 0.f), (float)(w - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(h - 1));
  t.x0 = (int)sx; t.y0 = (int)sy;
  t.x1 = min(t.x0 + 1, w - 1); t.y1 = min(t.y0 + 1, h - 1);
  t.fx = sx - (float)t.x0; t.fy = sy - (float)t.y0;
  return t;
}

static __device__ __forceinline__ float bilinear_fetch(const uint8_t* __restrict__ plane,
                                                       int stride, int comps,
                                                       const BilinearTaps& t) {
  const float p00 = plane[t.y0 * stride + t.x0 * comps];
  const float p01 = plane[t.y0 * stride + t.x1 * comps];
  const float p10 = plane[t.y1 * stride + t.x0 * comps];
  const float p11 = plane[t.y1 * stride + t.x1 * comps];
  const float top = p00 + (p01 - p00) * t.fx;
  const float bot = p10 + (p11 - p10) * t.fx;
  return top + (bot - top) * t.fy;
}

template <bool FROM_ARRAY, bool JFIF, int HS, int VS>
__global__ __launch_bounds__(256) void yuv420_clip_kernel(
    const uint8_t* __restrict__ buf, const long long* __restrict__ offs, void* __restrict__ out,
    YuvClipArgs a) {
  // grid = (pixel blocks of one frame, F, nclips): frame and clip are uniform
  // per block, so the base offset is one scalar load and no thread divides a
  // 64-bit pixel index (the cost of a flat grid: two such divisions per pixel)
  const int ohw = a.g.out_w * a.g.out_h;
  const int p = (int)(blockIdx.x * 256 + threadIdx.x);
  if (p >= ohw) return;
  const int f = (int)blockIdx.y, clip = (int)blockIdx.z;
  const long long i = ((long long)clip * a.F + f) * ohw + p;
  const int oy = p / a.g.out_w, ox = p - oy * a.g.out_w;
  const uint8_t* fr = buf + (FROM_ARRAY ? offs[clip] : a.offs[clip]) + f * a.frame_stride;
  const YuvBox box = FROM_ARRAY ? a.boxes_dev[clip] : a.boxes[clip];
  // the arithmetic below is nv12_clip_kernel's, expression for expression
  const float sx = box.x + ((float)ox + 0.5f) * (box.w / (float)a.g.out_w) - 0.5f;
  const float sy = box.y + ((float)oy + 0.5f) * (box.h / (float)a.g.out_h) - 0.5f;
  float yv, u, v;
  if constexpr (HS == 1 && VS == 1) {
    const BilinearTaps t = bilinear_taps(a.g.src_w, a.g.src_h, sx, sy);
    yv = bilinear_fetch(fr + a.y_off, a.y_stride, 1, t);
    u = bilinear_fetch(fr + a.u_off, a.u_stride, a.c_step, t) - 128.f;
    v = bilinear_fetch(fr + a.v_off, a.v_stride, a.c_step, t) - 128.f;
  } else {
    yv = nv12_sample(fr + a.y_off, a.g.src_w, a.g.src_h, a.y_stride, 1, 0, sx, sy);
    const float cx = HS == 2 ? (sx + 0.5f) * 0.5f - 0.5f : sx;
    const float cy = VS == 2 ? (sy + 0.5f) * 0.5f - 0.5f : sy;
    const int cw = chroma_dim<HS>(a.g.src_w, JFIF), ch = chroma_dim<VS>(a.g.src_h, JFIF);
    u = nv12_sample(fr + a.u_off, cw, ch, a.u_stride, a.c_step, 0, cx, cy) - 128.f;
    v = nv12_sample(fr + a.v_off, cw, ch, a.v_stride, a.c_step, 0, cx, cy) - 128.f;
  }
  clip_store<JFIF>(yv, u, v, a.norm, a.bf16, out, i);
}

// The antialiased form of yuv420_clip_kernel: the same inputs, mapping, colour
// and stores, but the triangle filter is widened by the downscale factor
// (PIL's BILINEAR resize, torch's antialias=True). Along one axis of one plane
// of n samples, output o of n_out from the box (start, size):
//   scale = size / n_out, fs = max(scale, 1), s = start + (o + 0.5) scale - 0.5
//   w_j = max(0, 1 - |j - s| / fs) for j = 0 .. n - 1, out = sum w_j p_j / sum w_j
// The support is cut at the plane's true samples (never the row stride or a
// JPEG surface's MCU padding) and the weights are renormalised; the launcher
// has checked that the box lies inside the frame, so no row of weights is empty.
//
// Separable inside the workgroup: a block owns AA_TH output rows x up to AA_TW
// output columns of one frame. Per plane it filters the source rows its band
// needs horizontally into LDS as fp32, AA_CH rows at a time (so LDS use does not
// depend on the scale), and every thread accumulates the vertical sums of its
// AA_PX output pixels in registers from LDS. Source reads are byte loads (Y4M
// frames are unaligned); a wave's loads of one tap walk one row segment.
// Weights are computed in fp32 here: no table, no upload. Every address is a
// function of geometry only, clamped to the plane.
#define AA_TW 128
#define AA_TH 8
#define AA_CH 32
#define AA_PX (AA_TW * AA_TH / 256)

static __device__ __forceinline__ float aa_coord(float start, float scale, int o) {
  return start + ((float)o + 0.5f) * scale - 0.5f;
}

// the samples inside the open support (s - fs, s + fs), cut to the plane; the
// weight's own max(0, .) still decides at an end that rounding moved
static __device__ __forceinline__ void aa_span(float s, float fs, int n, int& lo, int& hi) {
  lo = max((int)floorf(s - fs) + 1, 0);
  hi = min((int)ceilf(s + fs) - 1, n - 1);
}

// One plane of pw x ph samples (row stride `stride`, samples `step` bytes apart)
// resampled from the box (bx, by, bw, bh) at this thread's pixels: tile columns
// cx[k] (output column x0 + cx[k]) and output rows oy[k], k < AA_PX, oy < 0 for
// none. rows: the tile's output rows oy0 .. oy0 + th - 1. All threads of the
// block call this together (it synchronises).
static __device__ __forceinline__ void aa_plane(const uint8_t* __restrict__ plane, int pw, int ph,
                                                int stride, int step, float bx, float by,
                                                float bw, float bh, int out_w, int out_h,
                                                int x0, int tw, int oy0, int th,
                                                const int* cx, const int* oy,
                                                float* __restrict__ rows_lds, float* res) {
  const float scx = bw / (float)out_w, scy = bh / (float)out_h;
  const float fsx = fmaxf(scx, 1.f), fsy = fmaxf(scy, 1.f);
  const float ifx = 1.f / fsx, ify = 1.f / fsy;
  int band_lo, band_hi, unused;
  aa_span(aa_coord(by, scy, oy0), fsy, ph, band_lo, unused);
  aa_span(aa_coord(by, scy, oy0 + th - 1), fsy, ph, unused, band_hi);
  float acc[AA_PX], wsum[AA_PX], sy[AA_PX];
  int ylo[AA_PX], yhi[AA_PX];
#pragma unroll
  for (int k = 0; k < AA_PX; ++k) {
    acc[k] = 0.f;
    wsum[k] = 0.f;
    sy[k] = aa_coord(by, scy, max(oy[k], 0));
    aa_span(sy[k], fsy, ph, ylo[k], yhi[k]);
    if (oy[k] < 0) yhi[k] = -1;                      // no pixel: an empty span
  }
  for (int r0 = band_lo; r0 <= band_hi; r0 += AA_CH) {
    const int nrows = min(AA_CH, band_hi - r0 + 1);
    __syncthreads();                                 // the last readers of rows_lds are done
    for (int i = (int)threadIdx.x; i < nrows * tw; i += 256) {
      const int r = i / tw, c = i - r * tw;
      const float sx = aa_coord(bx, scx, x0 + c);
      int xlo, xhi;
      aa_span(sx, fsx, pw, xlo, xhi);
      const uint8_t* row = plane + (long long)(r0 + r) * stride;
      float a = 0.f, ws = 0.f;
      // four taps per trip so that four byte loads are in flight; a tap past xhi
      // reads sample xhi again with weight 0
      for (int j = xlo; j <= xhi; j += 4) {
        float p[4], w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) p[t] = (float)row[(long long)min(j + t, xhi) * step];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          w[t] = j + t <= xhi ? fmaxf(0.f, 1.f - fabsf((float)(j + t) - sx) * ifx) : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          a += w[t] * p[t];
          ws += w[t];
        }
      }
      // ws > 0 for every box the launcher lets through; the guard only keeps 0 / 0
      // out of LDS should that ever not hold. It is no edge handling.
      rows_lds[r * AA_TW + c] = ws > 0.f ? a / ws : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < AA_PX; ++k) {
      const int j1 = min(yhi[k], r0 + nrows - 1);
      for (int j = max(ylo[k], r0); j <= j1; ++j) {
        const float w = fmaxf(0.f, 1.f - fabsf((float)j - sy[k]) * ify);
        acc[k] += w * rows_lds[(j - r0) * AA_TW + cx[k]];
        wsum[k] += w;
      }
    }
  }
  // wsum is 0 only on idle lanes (oy < 0: no pixel, nothing stored): no 0 / 0 there
#pragma unroll
  for (int k = 0; k < AA_PX; ++k) res[k] = wsum[k] > 0.f ? acc[k] / wsum[k] : 0.f;
}

template <bool FROM_ARRAY, bool JFIF, int HS, int VS>
__global__ __launch_bounds__(256) void yuv420_clip_aa_kernel(
    const uint8_t* __restrict__ buf, const long long* __restrict__ offs, void* __restrict__ out,
    YuvClipArgs a) {
  // grid = (column tiles x row bands of one frame, F, nclips): frame and clip are
  // uniform per block, as in yuv420_clip_kernel
  __shared__ float rows_lds[AA_CH * AA_TW];
  const int col_tiles = (a.g.out_w + AA_TW - 1) / AA_TW;
  const int band = (int)blockIdx.x / col_tiles;
  const int x0 = ((int)blockIdx.x - band * col_tiles) * AA_TW;
  const int oy0 = band * AA_TH;
  const int tw = min(AA_TW, a.g.out_w - x0), th = min(AA_TH, a.g.out_h - oy0);
  const int f = (int)blockIdx.y, clip = (int)blockIdx.z;
  const uint8_t* fr = buf + (FROM_ARRAY ? offs[clip] : a.offs[clip]) + f * a.frame_stride;
  int cx[AA_PX], oy[AA_PX];
#pragma unroll
  for (int k = 0; k < AA_PX; ++k) {
    const int p = (int)threadIdx.x + 256 * k;       // pixel of the tile, row-major
    const int r = p / tw;
    cx[k] = p - r * tw;
    oy[k] = r < th ? oy0 + r : -1;
  }
  const int cw = chroma_dim<HS>(a.g.src_w, JFIF), ch = chroma_dim<VS>(a.g.src_h, JFIF);
  const YuvBox box = FROM_ARRAY ? a.boxes_dev[clip] : a.boxes[clip];
  float yv[AA_PX], u[AA_PX], v[AA_PX];
  aa_plane(fr + a.y_off, a.g.src_w, a.g.src_h, a.y_stride, 1, box.x, box.y,
           box.w, box.h, a.g.out_w, a.g.out_h, x0, tw, oy0, th, cx, oy, rows_lds, yv);
  // chroma sample j sits at luma 2 j + 0.5 along a subsampled axis: the chroma
  // box is the luma box / (HS, VS)
  const float hx = HS == 2 ? box.x * 0.5f : box.x;
  const float hy = VS == 2 ? box.y * 0.5f : box.y;
  const float hw = HS == 2 ? box.w * 0.5f : box.w;
  const float hh = VS == 2 ? box.h * 0.5f : box.h;
  aa_plane(fr + a.u_off, cw, ch, a.u_stride, a.c_step, hx, hy, hw, hh, a.g.out_w, a.g.out_h,
           x0, tw, oy0, th, cx, oy, rows_lds, u);
  aa_plane(fr + a.v_off, cw, ch, a.v_stride, a.c_step, hx, hy, hw, hh, a.g.out_w, a.g.out_h,
           x0, tw, oy0, th, cx, oy, rows_lds, v);
  const long long frame_px = ((long long)clip * a.F + f) * ((long long)a.g.out_w * a.g.out_h);
#pragma unroll
  for (int k = 0; k < AA_PX; ++k) {
    if (oy[k] < 0) continue;
    const long long i = frame_px + (long long)oy[k] * a.g.out_w + x0 + cx[k];
    clip_store<JFIF>(yv[k], u[k] - 128.f, v[k] - 128.f, a.norm, a.bf16, out, i);
  }
}

// one thread per 4 pixels: 12 bytes in (three aligned dword loads), 4 x 16 B
// out (8 bf16 per pixel, channels 3..7 zero); a tail thread goes per pixel
__global__ void preprocess_kernel(const uint8_t* __restrict__ in, uint16_t* __restrict__ out,
                                  long long npix, NormParams np) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i0 = q * 4;
  if (i0 >= npix) return;
  auto emit = [&](long long i, uint32_t r8, uint32_t g8, uint32_t b8) {
    const uint32_t r = f2bf_bits((float)r8 * np.scale[0] + np.shift[0]);
    const uint32_t g = f2bf_bits((float)g8 * np.scale[1] + np.shift[1]);
    const uint32_t b = f2bf_bits((float)b8 * np.scale[2] + np.shift[2]);
    *(uint4*)(out + i * 8) = make_uint4(r | (g << 16), b, 0u, 0u);
  };
  if (i0 + 4 <= npix) {
    const uint32_t* w = (const uint32_t*)(in + i0 * 3);   // 12-byte aligned groups
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    emit(i0 + 0, w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
    emit(i0 + 1, w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
    emit(i0 + 2, (w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
    emit(i0 + 3, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
  } else {
    for (long long i = i0; i < npix; ++i) {
      const uint8_t* px = in + i * 3;
      emit(i, px[0], px[1], px[2]);
    }
  }
}

// Stem repack for the pair-packed conv1 spatial conv (ops/conv.StemConv):
// NDHWC8 bf16 [F][H][W][8] (channels 0..2 used) -> zero-bordered
// [F][H+6][(W+6)/2][8], where packed pixel (y, xp) holds channels 0..3 of
// padded pixels 2xp and 2xp+1 (padded x = x + 3, padded y = y + 3). One
// thread = one 16-byte packed pixel: two 8-byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void stem_pack_kernel(const uint16_t* __restrict__ in,
                                                        uint16_t* __restrict__ out,
                                                        long long nout, int H, int W, int Hp,
                                                        int Wq) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nout) return;
  const long long r = i / Wq;
  const int xp = (int)(i - r * Wq);
  const long long f = r / Hp;
  const int yr = (int)(r - f * Hp) - 3;
  const int x0 = 2 * xp - 3;
  uint2 a = make_uint2(0u, 0u), b = make_uint2(0u, 0u);
  if (yr >= 0 && yr < H) {
    const uint16_t* row = in + (f * H + yr) * (long long)W * 8;
    if (x0 >= 0 && x0 < W) a = *(const uint2*)(row + (long long)x0 * 8);
    if (x0 + 1 >= 0 && x0 + 1 < W) b = *(const uint2*)(row + (long long)(x0 + 1) * 8);
  }
  *(uint4*)(out + i * 8) = make_uint4(a.x, a.y, b.x, b.y);
}

// preprocess fused with the stem repack: uint8 [F][H][W][3] -> zero-bordered
// pair-packed bf16 [F][H+6][(W+6)/2][8] (the layout of stem_pack_kernel), so
// the decoder writes the stem conv's input directly. One thread = one packed
// pixel: up to 6 byte loads, one 16-byte store; the border is written as zero.
__global__ __launch_bounds__(256) void preprocess_packed_kernel(const uint8_t* __restrict__ in,
                                                                uint16_t* __restrict__ out,
                                                                long long nout, int H, int W,
                                                                int Hp, int Wq, NormParams np) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nout) return;
  const long long r = i / Wq;
  const int xp = (int)(i - r * Wq);
  const long long f = r / Hp;
  const int yr = (int)(r - f * Hp) - 3;
  const int x0 = 2 * xp - 3;
  uint32_t v[4] = {0u, 0u, 0u, 0u};
  if (yr >= 0 && yr < H) {
    const uint8_t* row = in + (f * H + yr) * (long long)W * 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int x = x0 + h;
      if (x >= 0 && x < W) {
        const uint8_t* px = row + (long long)x * 3;
        const uint32_t rr = f2bf_bits((float)px[0] * np.scale[0] + np.shift[0]);
        const uint32_t gg = f2bf_bits((float)px[1] * np.scale[1] + np.shift[1]);
        const uint32_t bb = f2bf_bits((float)px[2] * np.scale[2] + np.shift[2]);
        v[2 * h] = rr | (gg << 16);
        v[2 * h + 1] = bb;
      }
    }
  }
  *(uint4*)(out + i * 8) = make_uint4(v[0], v[1], v[2], v[3]);
}

// Head, part 1: average pool. x: [N][S][Cs] bf16 (NDHWC, S = T*H*W) ->
// pooled [N][C] f32. One thread per (clip, channel pair); the S-loop is
// unrolled so 7 loads are in flight per thread (a pooled sum is a chain of
// dependent adds, but its loads are independent).
__global__ __launch_bounds__(256) void head_pool_kernel(const uint16_t* __restrict__ x,
                                                        float* __restrict__ pooled, int N,
                                                        int S, int C, int Cs) {
  const int cp = C / 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * cp) return;
  const int n = (int)(i / cp);
  const int c = (int)(i - (long long)n * cp) * 2;
  const uint16_t* xc = x + (size_t)n * S * Cs + c;
  float s0 = 0.f, s1 = 0.f;
  int s = 0;
  for (; s + 7 <= S; s += 7) {
    uint32_t v[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = *(const uint32_t*)(xc + (size_t)(s + j) * Cs);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      s0 += __uint_as_float(v[j] << 16);
      s1 += __uint_as_float(v[j] & 0xFFFF0000u);
    }
  }
  for (; s < S; ++s) {
    const uint32_t v = *(const uint32_t*)(xc + (size_t)s * Cs);
    s0 += __uint_as_float(v << 16);
    s1 += __uint_as_float(v & 0xFFFF0000u);
  }
  const float inv = 1.0f / (float)S;
  *(float2*)(pooled + (size_t)n * C + c) = make_float2(s0 * inv, s1 * inv);
}

// Head, part 2: linear. pooled [N][C] f32, wt: [C][ncls] f32 (TRANSPOSED linear
// weight), out: [N][ncls] f32. Grid = (ceil(ncls / 64), ceil(N / 16)); a
// block stages its 16 clips' pooled rows in LDS. The C reduction is split
// over the 4 waves (a quarter of C each, 16 weight loads in flight per lane)
// so the dependent-load chain is C/64 deep instead of C; lane l computes class
// 64 * blockIdx.x + l for all 16 clips and the 4 partial sums meet in LDS.
#define HEAD_CLIPS 16
#define HEAD_CLS 64
__global__ __launch_bounds__(256) void head_linear_kernel(const float* __restrict__ pooled_g,
                                                          const float* __restrict__ wt,
                                                          const float* __restrict__ bias,
                                                          float* __restrict__ out, int N,
                                                          int C, int ncls) {
  extern __shared__ float smem_f[];                  // pooled [16][C] | partial [4][16][64]
  float* pooled = smem_f;
  float* partial = smem_f + HEAD_CLIPS * C;
  const int n0 = blockIdx.y * HEAD_CLIPS;
  const int nb = min(HEAD_CLIPS, N - n0);
  for (int idx = threadIdx.x; idx < HEAD_CLIPS * C / 4; idx += blockDim.x) {
    const int j = idx / (C / 4);
    const float4 v = j < nb ? *(const float4*)(pooled_g + (size_t)(n0 + j) * C +
                                                (idx - j * (C / 4)) * 4)
                            : make_float4(0.f, 0.f, 0.f, 0.f);
    *(float4*)(pooled + idx * 4) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int o = blockIdx.x * HEAD_CLS + lane;
  const int oc = min(o, ncls - 1);                   // clamped: every lane joins the reduce
  const int cq = C / 4;
  const int c0 = wave * cq;
  float acc[HEAD_CLIPS];
#pragma unroll
  for (int j = 0; j < HEAD_CLIPS; ++j) acc[j] = 0.f;
  for (int c = c0; c < c0 + cq; c += 16) {
    float w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w[u] = c + u < c0 + cq ? wt[(size_t)(c + u) * ncls + oc] : 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (c + u >= c0 + cq) break;
#pragma unroll
      for (int j = 0; j < HEAD_CLIPS; ++j) acc[j] += w[u] * pooled[j * C + c + u];
    }
  }
#pragma unroll
  for (int j = 0; j < HEAD_CLIPS; ++j) partial[(wave * HEAD_CLIPS + j) * HEAD_CLS + lane] = acc[j];
  __syncthreads();
  // 256 threads finish 16 clips x 64 classes: 4 outputs each
  for (int q = threadIdx.x; q < HEAD_CLIPS * HEAD_CLS; q += 256) {
    const int j = q / HEAD_CLS, l = q - j * HEAD_CLS;
    const int oo = blockIdx.x * HEAD_CLS + l;
    if (j < nb && oo < ncls) {
      float v = bias[oo];
#pragma unroll
      for (int w4 = 0; w4 < 4; ++w4) v += partial[(w4 * HEAD_CLIPS + j) * HEAD_CLS + l];
      out[(size_t)(n0 + j) * ncls + oo] = v;
    }
  }
}

// logits: [nclips][ncls]; offsets: [nvid+1] clip ranges; sums: [nvid][ncls]; arg: [nvid]
__global__ __launch_bounds__(256) void video_reduce_kernel(const float* __restrict__ logits,
                                                           const int* __restrict__ offsets,
                                                           float* __restrict__ sums,
                                                           int* __restrict__ argmax, int ncls) {
  __shared__ float bv[256];
  __shared__ int bi[256];
  const int v = blockIdx.x;
  const int c0 = offsets[v], c1 = offsets[v + 1];
  float best = -INFINITY;
  int besti = 0x7FFFFFFF;
  for (int o = threadIdx.x; o < ncls; o += 256) {
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += logits[(size_t)c * ncls + o];
    if (sums) sums[(size_t)v * ncls + o] = s;
    if (s > best || (s == best && o < besti)) { best = s; besti = o; }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = besti;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if (threadIdx.x < step) {
      const float ov = bv[threadIdx.x + step];
      const int oi = bi[threadIdx.x + step];
      if (ov > bv[threadIdx.x] || (ov == bv[threadIdx.x] && oi < bi[threadIdx.x])) {
        bv[threadIdx.x] = ov;
        bi[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) argmax[v] = (c1 > c0) ? bi[0] : -1;
}


// fp32 path (reference precision): uint8 NFHWC3 -> normalised fp32 NDHWC4
// (channel 3 zero), so one 16-byte chunk is one pixel and the stem conv's K
// is 7*7*4 = 196. One thread per 4 pixels: three dword loads, 4 x 16 B out.
__global__ void preprocess_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out,
                                      long long npix, NormParams np) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i0 = q * 4;
  if (i0 >= npix) return;
  auto emit = [&](long long i, uint32_t r8, uint32_t g8, uint32_t b8) {
    *(float4*)(out + i * 4) = make_float4((float)r8 * np.scale[0] + np.shift[0],
                                          (float)g8 * np.scale[1] + np.shift[1],
                                          (float)b8 * np.scale[2] + np.shift[2], 0.f);
  };
  if (i0 + 4 <= npix) {
    const uint32_t* w = (const uint32_t*)(in + i0 * 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    emit(i0 + 0, w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
    emit(i0 + 1, w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
    emit(i0 + 2, (w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
    emit(i0 + 3, (w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
  } else {
    for (long long i = i0; i < npix; ++i) {
      const uint8_t* px = in + i * 3;
      emit(i, px[0], px[1], px[2]);
    }
  }
}

// fp32 head, part 1: average pool of an fp32 NDHWC tensor. One thread per
// (clip, 4 channels): 16-byte loads, 7 in flight per thread.
__global__ __launch_bounds__(256) void head_pool_f32_kernel(const float* __restrict__ x,
                                                            float* __restrict__ pooled, int N,
                                                            int S, int C, int Cs) {
  const int cq = C / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * cq) return;
  const int n = (int)(i / cq);
  const int c = (int)(i - (long long)n * cq) * 4;
  const float* xc = x + (size_t)n * S * Cs + c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  int t = 0;
  for (; t + 7 <= S; t += 7) {
    float4 v[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = *(const float4*)(xc + (size_t)(t + j) * Cs);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w;
    }
  }
  for (; t < S; ++t) {
    const float4 v = *(const float4*)(xc + (size_t)t * Cs);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  const float inv = 1.0f / (float)S;
  *(float4*)(pooled + (size_t)n * C + c) = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
}

// rnb_yuv_to_clip_boxes' choice among the instantiations of the two clip kernels
template <bool FROM_ARRAY, bool JFIF, int HS, int VS>
static void yuv_box_run(bool aa, dim3 grid, hipStream_t stream, const uint8_t* buf,
                        const long long* table, void* out, const YuvClipArgs& a) {
  if (aa)
    hipLaunchKernelGGL((yuv420_clip_aa_kernel<FROM_ARRAY, JFIF, HS, VS>), grid, dim3(256), 0,
                       stream, buf, table, out, a);
  else
    hipLaunchKernelGGL((yuv420_clip_kernel<FROM_ARRAY, JFIF, HS, VS>), grid, dim3(256), 0,
                       stream, buf, table, out, a);
}

template <bool FROM_ARRAY, bool JFIF>
static void yuv_box_run_sampling(int sampling, bool aa, dim3 grid, hipStream_t stream,
                                 const uint8_t* buf, const long long* table, void* out,
                                 const YuvClipArgs& a) {
  if (sampling == 0) yuv_box_run<FROM_ARRAY, JFIF, 2, 2>(aa, grid, stream, buf, table, out, a);
  else if (sampling == 1) yuv_box_run<FROM_ARRAY, JFIF, 2, 1>(aa, grid, stream, buf, table, out, a);
  else yuv_box_run<FROM_ARRAY, JFIF, 1, 1>(aa, grid, stream, buf, table, out, a);
}

extern "C" {

int rnb_clipgen_u8(void* out, const int* vids, const int* starts, int nclips, int F, int H,
                   int W, hipStream_t stream) {
  if (nclips <= 0) return 0;
  if (((long long)H * W) % 16 != 0) return -2;      // 16-pixel runs must not cross frames
  const long long total = (long long)nclips * F * H * W;
  const long long threads = (total + 15) / 16;
  const int block = 256;
  const long long grid = (threads + block - 1) / block;
  hipLaunchKernelGGL(clipgen_u8_kernel, dim3((unsigned)grid), dim3(block), 0, stream,
                     (uint8_t*)out, vids, starts, nclips, F, H, W);
  return (int)hipGetLastError();
}

// F * step_p must fit an int: the kernels compute (f * step_p) / step_q in 32 bits
static bool clipgen_step_ok(int F, int step_p, int step_q) {
  return F >= 1 && F <= 65535 && step_p >= 1 && step_q >= 1 &&
         (long long)F * step_p <= 2147483647LL;
}

int rnb_clipgen_video_step(void* out, int vid, const int* starts, int nclips, int F, int H,
                           int W, int step_p, int step_q, hipStream_t stream) {
  if (nclips <= 0) return 0;
  if (nclips > CLIPGEN_MAX_CLIPS) return -3;
  if (((long long)H * W) % 16 != 0) return -2;
  if (!clipgen_step_ok(F, step_p, step_q)) return -2;
  ClipgenArgs a;
  a.vid = vid;
  a.nclips = nclips;
  a.step_p = step_p;
  a.step_q = step_q;
  for (int i = 0; i < CLIPGEN_MAX_CLIPS; ++i) a.starts[i] = i < nclips ? starts[i] : 0;
  const long long threads = ((long long)nclips * F * H * W + 15) / 16;
  hipLaunchKernelGGL(clipgen_video_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     stream, (uint8_t*)out, a, F, H, W);
  return (int)hipGetLastError();
}

int rnb_clipgen_video(void* out, int vid, const int* starts, int nclips, int F, int H, int W,
                      hipStream_t stream) {
  return rnb_clipgen_video_step(out, vid, starts, nclips, F, H, W, 1, 1, stream);
}

int rnb_nv12gen_video_step(void* out, int vid, const int* starts, int nclips, int F, int H,
                           int W, int step_p, int step_q, hipStream_t stream) {
  if (nclips <= 0) return 0;
  if (nclips > CLIPGEN_MAX_CLIPS || H % 2 || W % 2) return -3;
  if (!clipgen_step_ok(F, step_p, step_q)) return -2;
  ClipgenArgs a;
  a.vid = vid;
  a.nclips = nclips;
  a.step_p = step_p;
  a.step_q = step_q;
  for (int i = 0; i < CLIPGEN_MAX_CLIPS; ++i) a.starts[i] = i < nclips ? starts[i] : 0;
  const long long bytes = (long long)nclips * F * H * W * 3 / 2;
  const long long threads = (bytes + 15) / 16;
  hipLaunchKernelGGL(nv12gen_kernel<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256),
                     0, stream, (uint8_t*)out, a, (const int*)nullptr, (const int*)nullptr, F, H,
                     W);
  return (int)hipGetLastError();
}

int rnb_nv12gen_video(void* out, int vid, const int* starts, int nclips, int F, int H, int W,
                      hipStream_t stream) {
  return rnb_nv12gen_video_step(out, vid, starts, nclips, F, H, W, 1, 1, stream);
}

// batched form (per-clip video id / start frame in device arrays: graph-capturable)
int rnb_nv12gen(void* out, const int* vids, const int* starts, int nclips, int F, int H, int W,
                hipStream_t stream) {
  if (nclips <= 0) return 0;
  if (H % 2 || W % 2) return -3;
  ClipgenArgs a;
  a.vid = 0;
  a.nclips = nclips;
  a.step_p = a.step_q = 1;
  const long long bytes = (long long)nclips * F * H * W * 3 / 2;
  const long long threads = (bytes + 15) / 16;
  hipLaunchKernelGGL(nv12gen_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     stream, (uint8_t*)out, a, vids, starts, F, H, W);
  return (int)hipGetLastError();
}

// nv12: [frames][H*3/2][W] bytes -> out: [frames][oh][ow][4] fp32 or [..][8] bf16
int rnb_nv12_to_clip(const void* nv12, void* out, long long frames, int src_w, int src_h,
                     int out_w, int out_h, const float* crop, const float* mean,
                     const float* stdv, int bf16, hipStream_t stream) {
  if (frames <= 0) return 0;
  if (src_w % 2 || src_h % 2 || out_w <= 0 || out_h <= 0) return -2;
  if (((uintptr_t)out & 15u) != 0) return -2;
  Nv12ClipArgs a;
  a.g.src_w = src_w; a.g.src_h = src_h; a.g.out_w = out_w; a.g.out_h = out_h;
  a.crop_x = crop[0]; a.crop_y = crop[1]; a.crop_w = crop[2]; a.crop_h = crop[3];
  a.norm = norm_params(mean, stdv);
  a.bf16 = bf16;
  const long long npix = frames * out_w * out_h;
  hipLaunchKernelGGL(nv12_clip_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0,
                     stream, (const uint8_t*)nv12, out, npix, a);
  return (int)hipGetLastError();
}

// everything the clip launcher checks but the crop boxes (0: fine). tables_ok:
// the rows fit the kernel arguments, or their tables are in device memory.
static int yuv_clip_check(long long buf_len, const long long* offs, int nclips, bool tables_ok,
                          int F, int src_w, int src_h, long long frame_stride,
                          const long long* plane_off, const int* plane_stride, int c_step,
                          const void* out, int out_w, int out_h, int matrix, int filter,
                          int sampling) {
  if (matrix != 0 && matrix != 1) return -2;
  if (sampling < 0 || sampling > 2) return -2;
  const int hs = sampling == 2 ? 1 : 2, vs = sampling == 0 ? 2 : 1;
  if (F <= 0 || src_w < 1 || src_h < 1 || out_w <= 0 || out_h <= 0) return -2;
  if (matrix == 0 && ((hs == 2 && src_w % 2) || (vs == 2 && src_h % 2))) return -2;
  if (((uintptr_t)out & 15u) != 0 || (c_step != 1 && c_step != 2)) return -2;
  if (!tables_ok) return -3;
  // every byte nv12_sample can touch lies inside its frame (int indexing there)
  if (frame_stride <= 0 || frame_stride > 0x7FFFFFFFLL) return -4;
  const int cw = hs == 2 ? (src_w + matrix) / 2 : src_w;
  const int ch = vs == 2 ? (src_h + matrix) / 2 : src_h;
  for (int p = 0; p < 3; ++p) {
    if (plane_off[p] < 0 || plane_stride[p] <= 0) return -4;
    const long long row = p == 0 ? src_w : (long long)(cw - 1) * c_step + 1;
    const long long rows = p == 0 ? src_h : ch;
    if (plane_off[p] + (rows - 1) * plane_stride[p] + row > frame_stride) return -4;
  }
  for (int c = 0; c < nclips; ++c)
    if (offs[c] < 0 || offs[c] + (long long)F * frame_stride > buf_len) return -4;
  const long long ohw = (long long)out_w * out_h;
  if (ohw > 0x7FFFFF00LL || F > 65535 || nclips > 65535) return -2;    // grid limits
  const long long tiles = (long long)((out_w + AA_TW - 1) / AA_TW) * ((out_h + AA_TH - 1) / AA_TH);
  if (filter && tiles > 0x7FFFFFFFLL) return -2;
  return 0;
}

// the antialias kernel's condition on a crop box: inside [0, src_w] x [0, src_h],
// summed in double (no row of weights can then be empty)
static bool yuv_clip_box_inside(const float* b, int src_w, int src_h) {
  return b[0] >= 0.f && b[1] >= 0.f && b[2] > 0.f && b[3] > 0.f &&
         (double)b[0] + b[2] <= src_w && (double)b[1] + b[3] <= src_h;
}

static dim3 yuv_clip_grid(int filter, int out_w, int out_h, int F, int nclips) {
  const long long ohw = (long long)out_w * out_h;
  const long long tiles = (long long)((out_w + AA_TW - 1) / AA_TW) * ((out_h + AA_TH - 1) / AA_TH);
  return dim3((unsigned)(filter ? tiles : (ohw + 255) / 256), (unsigned)F, (unsigned)nclips);
}

// buf: buf_len uploaded bytes; row c of the launch reads the F frames that start
// at offs[c] (host copy, checked here) and are frame_stride bytes apart, through
// the crop box boxes[c] = (x, y, w, h), so the views of one clip share its
// uploaded span (rows may repeat an offset, in any order). plane_off /
// plane_stride: byte offset within a frame and row stride of Y, U, V; c_step:
// bytes between chroma samples (1 planar, 2 interleaved). out:
// [nclips][F][oh][ow][4] fp32 or [..][8] bf16. Up to YUV_BOX_MAX_ROWS rows travel
// in the kernel arguments; more need offs_dev AND boxes_dev, both tables in
// device memory (-3 otherwise). -4: a frame or a span would reach outside its
// frame stride / the buffer (nothing is launched).
// matrix: 0 BT.601 video range, 1 full-range JFIF (any size).
// filter: 0 the two-tap bilinear kernel, which takes any box, 1 the antialiased
// triangle filter (yuv420_clip_aa_kernel), which needs every box inside
// [0, src_w] x [0, src_h] (a row of weights could be empty), else -5 and nothing
// is launched.
// sampling: 0 4:2:0 (luma factors 2x2), 1 4:2:2 (2x1), 2 4:4:4 (1x1); the chroma
// planes are ceil(w / Hs) x ceil(h / Vs) under JFIF and w / Hs x h / Vs under
// BT.601, which needs an even size only along an axis with factor 2.
// Anything else in matrix, filter or sampling: -2.
int rnb_yuv_to_clip_boxes(const void* buf, long long buf_len, const long long* offs,
                          const void* offs_dev, int nclips, int F, int src_w, int src_h,
                          long long frame_stride, const long long* plane_off,
                          const int* plane_stride, int c_step, void* out, int out_w, int out_h,
                          const float* boxes, const void* boxes_dev, const float* mean,
                          const float* stdv, int bf16, int matrix, int filter, int sampling,
                          hipStream_t stream) {
  if (nclips <= 0) return 0;
  if (filter != 0 && filter != 1) return -2;
  const bool in_args = nclips <= YUV_BOX_MAX_ROWS;
  const int rc = yuv_clip_check(buf_len, offs, nclips, in_args || (offs_dev && boxes_dev), F,
                                src_w, src_h, frame_stride, plane_off, plane_stride, c_step, out,
                                out_w, out_h, matrix, filter, sampling);
  if (rc) return rc;
  if (((uintptr_t)boxes_dev & 15u) != 0) return -2;         // 16-byte box loads
  if (filter)
    for (int c = 0; c < nclips; ++c)
      if (!yuv_clip_box_inside(boxes + 4 * c, src_w, src_h)) return -5;
  YuvClipArgs a;
  a.g.src_w = src_w; a.g.src_h = src_h; a.g.out_w = out_w; a.g.out_h = out_h;
  a.norm = norm_params(mean, stdv);
  a.bf16 = bf16;
  a.F = F; a.c_step = c_step; a.frame_stride = frame_stride;
  a.y_off = plane_off[0]; a.u_off = plane_off[1]; a.v_off = plane_off[2];
  a.y_stride = plane_stride[0]; a.u_stride = plane_stride[1]; a.v_stride = plane_stride[2];
  a.boxes_dev = in_args ? (const YuvBox*)nullptr : (const YuvBox*)boxes_dev;
  for (int c = 0; c < YUV_BOX_MAX_ROWS; ++c) {
    const bool live = in_args && c < nclips;
    a.offs[c] = live ? offs[c] : 0;
    a.boxes[c].x = live ? boxes[4 * c] : 0.f;
    a.boxes[c].y = live ? boxes[4 * c + 1] : 0.f;
    a.boxes[c].w = live ? boxes[4 * c + 2] : 0.f;
    a.boxes[c].h = live ? boxes[4 * c + 3] : 0.f;
  }
  const long long* table = in_args ? (const long long*)nullptr : (const long long*)offs_dev;
  const dim3 grid = yuv_clip_grid(filter, out_w, out_h, F, nclips);
  const uint8_t* src = (const uint8_t*)buf;
  const bool aa = filter != 0;
  if (in_args) {
    if (matrix) yuv_box_run_sampling<false, true>(sampling, aa, grid, stream, src, table, out, a);
    else yuv_box_run_sampling<false, false>(sampling, aa, grid, stream, src, table, out, a);
  } else {
    if (matrix) yuv_box_run_sampling<true, true>(sampling, aa, grid, stream, src, table, out, a);
    else yuv_box_run_sampling<true, false>(sampling, aa, grid, stream, src, table, out, a);
  }
  return (int)hipGetLastError();
}

int rnb_preprocess(const void* in, void* out, long long npix, const float* mean,
                   const float* stdv, hipStream_t stream) {
  if (npix <= 0) return 0;
  const NormParams np = norm_params(mean, stdv);
  if (((uintptr_t)in & 3u) != 0) return -2;         // dword loads of 4-pixel groups
  const int block = 256;
  const long long grid = ((npix + 3) / 4 + block - 1) / block;
  hipLaunchKernelGGL(preprocess_kernel, dim3((unsigned)grid), dim3(block), 0, stream,
                     (const uint8_t*)in, (uint16_t*)out, npix, np);
  return (int)hipGetLastError();
}

// w: TRANSPOSED linear weight [C][ncls]; pooled: [N][C] f32 scratch
int rnb_head(const void* x, const float* w, const float* b, float* out, float* pooled, int N,
             int S, int C, int Cs, int ncls, hipStream_t stream) {
  if (N <= 0) return 0;
  if (C % 4 != 0 || Cs % 2 != 0 || Cs < C || !pooled) return -2;
  const size_t lds = ((size_t)HEAD_CLIPS * C + 4 * HEAD_CLIPS * HEAD_CLS) * sizeof(float);
  if (lds > 64 * 1024 || C % 16 != 0) return -3;
  const long long threads = (long long)N * (C / 2);
  hipLaunchKernelGGL(head_pool_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     stream, (const uint16_t*)x, pooled, N, S, C, Cs);
  const dim3 grid((ncls + HEAD_CLS - 1) / HEAD_CLS, (N + HEAD_CLIPS - 1) / HEAD_CLIPS);
  hipLaunchKernelGGL(head_linear_kernel, grid, dim3(256), lds, stream, pooled, w, b, out, N, C,
                     ncls);
  return (int)hipGetLastError();
}

int rnb_video_reduce(const float* logits, const int* offsets, float* sums, int* argmax,
                     int nvid, int ncls, hipStream_t stream) {
  if (nvid <= 0) return 0;
  hipLaunchKernelGGL(video_reduce_kernel, dim3(nvid), dim3(256), 0, stream, logits, offsets,
                     sums, argmax, ncls);
  return (int)hipGetLastError();
}

// in: [frames][H][W][8] bf16, out: [frames][H+6][(W+6)/2][8] bf16 (W even)
int rnb_stem_pack(const void* in, void* out, long long frames, int H, int W,
                  hipStream_t stream) {
  if (frames <= 0) return 0;
  if (W % 2 != 0 || H <= 0 || W <= 0) return -2;
  if ((((uintptr_t)in) & 7u) != 0 || (((uintptr_t)out) & 15u) != 0) return -2;
  const int Hp = H + 6, Wq = (W + 6) / 2;
  const long long nout = frames * Hp * Wq;
  hipLaunchKernelGGL(stem_pack_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0,
                     stream, (const uint16_t*)in, (uint16_t*)out, nout, H, W, Hp, Wq);
  return (int)hipGetLastError();
}

// in: uint8 [frames][H][W][3], out: [frames][H+6][(W+6)/2][8] bf16 (W even)
int rnb_preprocess_packed(const void* in, void* out, long long frames, int H, int W,
                          const float* mean, const float* stdv, hipStream_t stream) {
  if (frames <= 0) return 0;
  if (W % 2 != 0 || H <= 0 || W <= 0) return -2;
  if ((((uintptr_t)out) & 15u) != 0) return -2;
  const NormParams np = norm_params(mean, stdv);
  const int Hp = H + 6, Wq = (W + 6) / 2;
  const long long nout = frames * Hp * Wq;
  hipLaunchKernelGGL(preprocess_packed_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256),
                     0, stream, (const uint8_t*)in, (uint16_t*)out, nout, H, W, Hp, Wq, np);
  return (int)hipGetLastError();
}

int rnb_preprocess_f32(const void* in, void* out, long long npix, const float* mean,
                       const float* stdv, hipStream_t stream) {
  if (npix <= 0) return 0;
  const NormParams np = norm_params(mean, stdv);
  if (((uintptr_t)in & 3u) != 0 || ((uintptr_t)out & 15u) != 0) return -2;
  const int block = 256;
  const long long grid = ((npix + 3) / 4 + block - 1) / block;
  hipLaunchKernelGGL(preprocess_f32_kernel, dim3((unsigned)grid), dim3(block), 0, stream,
                     (const uint8_t*)in, (float*)out, npix, np);
  return (int)hipGetLastError();
}

// x: fp32 [N][S][Cs]; w: TRANSPOSED linear weight [C][ncls]; pooled: [N][C] scratch
int rnb_head_f32(const float* x, const float* w, const float* b, float* out, float* pooled,
                 int N, int S, int C, int Cs, int ncls, hipStream_t stream) {
  if (N <= 0) return 0;
  if (C % 16 != 0 || Cs % 4 != 0 || Cs < C || !pooled) return -2;
  const size_t lds = ((size_t)HEAD_CLIPS * C + 4 * HEAD_CLIPS * HEAD_CLS) * sizeof(float);
  if (lds > 64 * 1024) return -3;
  const long long threads = (long long)N * (C / 4);
  hipLaunchKernelGGL(head_pool_f32_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256),
                     0, stream, x, pooled, N, S, C, Cs);
  const dim3 grid((ncls + HEAD_CLS - 1) / HEAD_CLS, (N + HEAD_CLIPS - 1) / HEAD_CLIPS);
  hipLaunchKernelGGL(head_linear_kernel, grid, dim3(256), lds, stream, pooled, w, b, out, N, C,
                     ncls);
  return (int)hipGetLastError();
}

}  // extern "C"

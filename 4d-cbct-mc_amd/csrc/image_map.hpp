// image_map.hpp -- interface of the CT -> material mapping kernels (image_map.hip), used by engine_geometry.cpp and model_device.cpp.
//
// THE MAPPING RULE (the one statement of it in the C sources; DESIGN.md row f8 repeats it for readers of the documents).  It is the
// closed form of the reference's fixed mapper pipeline (cbctmc/mc/geometry.py:35-234 the mappers, :237-309 the pipeline and its order).
// Classes, in this order (ImageClass): air, soft_tissue, red_marrow, bone_020, bone_050, bone_100, lung, liver, stomach_intestines,
// muscle_tissue, adipose, blood.  s_k = "segmentation k > 0" (ImageSegmentation: body, bone, lung, liver, stomach, muscle, fat, lung
// vessels), v = the image value (int16 or float32) converted to float32 (exact for int16), t = the three float32 thresholds
// {150, 300, -900}.  The comparisons are exactly the ones written, so a NaN fails all of them, as in numpy.  Later lines overwrite
// earlier ones; a line whose segmentation is absent (null) is skipped:
//   1 body     s_body -> soft_tissue, else air                       (every voxel)
//   2 bone     where s_bone:  v < t0 -> red_marrow;  t0 <= v && v < t1 -> bone_020;
//              v >= t1 -> bone_050, or bone_100 on the one-voxel OUTLINE of the bone mask: in the mask but not in its erosion by the
//              6-neighbour cross, voxels outside the volume counting as background (scipy.ndimage.binary_erosion's defaults)
//   3 lung -> lung   4 liver -> liver   5 stomach -> stomach_intestines   6 muscle -> muscle_tissue   7 fat -> adipose
//   8 air      s_body && v < t2 -> air
//   9 vessels  -> blood
// A voxel no executed line touches is UNMAPPED (only possible without a body segmentation); the callers refuse such a volume.
// The rule is a function of the voxel and the bone bit of its six face neighbours, and the cross is symmetric under the rot90 between
// the two frames, so it may be evaluated in either frame.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace mcgpu {

constexpr int kImageClasses = 12, kImageSegmentations = 8;
constexpr unsigned char kImageUnmapped = 0xFF;
enum ImageClass : int { kClassAir = 0, kClassSoftTissue, kClassRedMarrow, kClassBone020, kClassBone050, kClassBone100, kClassLung, kClassLiver,
                        kClassStomach, kClassMuscle, kClassAdipose, kClassBlood };
enum ImageSegmentation : int { kSegBody = 0, kSegBone, kSegLung, kSegLiver, kSegStomach, kSegMuscle, kSegFat, kSegVessels };
// words of ImageMapArgs::stats: [c] voxels of class c, [12 + c] the smallest linear [z][y][x] index of the engine's frame at which class c
// occurs (0xFFFFFFFF: nowhere), [24] unmapped voxels.  The caller initialises them (image_map_stats_init).
constexpr int kImageStatWords = 2 * kImageClasses + 1;

struct ImageMapArgs {
  const void* image;  // int16 or float32 (image_is_f32), device memory, laid out like the segmentations
  int image_is_f32;
  const unsigned char* seg[kImageSegmentations];  // device memory; null: the line is skipped
  float threshold[3];                             // red_marrow | bone_020 | bone_050 boundaries, then the air line's
  unsigned int* stats;                            // kImageStatWords words, device memory
};

inline void image_map_stats_init(unsigned int* words) {
  for (int i = 0; i < kImageStatWords; ++i) words[i] = (i >= kImageClasses && i < 2 * kImageClasses) ? 0xFFFFFFFFu : 0u;
}

// The class of every voxel into a 4x4x4-TILED u8 volume of the engine's frame (device_model.hpp: tiled_voxel; the padding voxels of
// edge tiles repeat the tile's first voxel, as model_device.cpp: tiled_volume writes them).  frame 0: inputs [nz][ny][nx]; frame 1:
// inputs [gx][gy][gz] = [ny][nx][nz], engine voxel (x, y, z) = input voxel (ny - 1 - y, x, z).  nx ny nz < 2^31.
hipError_t launch_image_map_tiled(const ImageMapArgs& a, int frame, int nx, int ny, int nz, unsigned char* classes_tiled, int num_cus, hipStream_t stream);
// The mapping alone, in the inputs' own layout [n2][n1][n0] (n0 fastest): material number and density of every voxel's class from
// the 12-entry table; an unmapped voxel gets (0, 0).
hipError_t launch_image_map_plain(const ImageMapArgs& a, int n0, int n1, int n2, const unsigned char material[kImageClasses], const float density[kImageClasses],
                                  unsigned char* material_out, float* density_out, int num_cus, hipStream_t stream);
// out[i] = lut[in[i]] over `bytes` bytes (a multiple of 16; both 16-byte aligned): classes -> palette indices
hipError_t launch_image_remap(const unsigned char* in, unsigned char* out, size_t bytes, const unsigned char lut[16], hipStream_t stream);

}  // namespace mcgpu

// smhip/pcd.h -- the static map's file: what pcl::io::savePCDFileBinary writes for a pcl::PointCloud<pcl::PointXYZI> or
// <pcl::PointXYZRGB> (PCL 1.8, the version the reference includes; called from MultiResolutionVoxelMap::OutputToPointCloud,
// builder/multi_resolution_voxel_map.cc:217-242), without PCL and without HIP.
//
//   an 11-line v0.7 header            # .PCD v0.7 - Point Cloud Data file format / VERSION 0.7 / FIELDS x y z intensity (or rgb) /
//                                     SIZE 4 4 4 4 / TYPE F F F F / COUNT 1 1 1 1 / WIDTH n / HEIGHT 1 / VIEWPOINT 0 0 0 1 0 0 0 /
//                                     POINTS n / DATA binary
//   n rows of 16 bytes                x y z and the fourth field as float32, packed (PCL copies the named fields only, not the
//                                     padding of its point types); XYZRGB's `rgb` is a float holding the packed colour's bits
//
// An empty cloud writes no file and prints the reference's warning (:226-228).  DATA binary_compressed (the reference's default
// compress = true, LZF) is not written: callers asking for it get DATA binary and a warning.
#pragma once

#include <cstdio>
#include <string>

namespace smhip {
namespace pcd {

// The header PCL's generateHeader<PointT> + "DATA binary\n" produce for n points of one of the two layouts.
inline std::string BinaryHeader(size_t n, bool rgb) {
  const std::string w = std::to_string(n);
  return std::string("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z ") + (rgb ? "rgb" : "intensity") +
         "\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH " + w + "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " + w + "\nDATA binary\n";
}

// rows: n x 4 floats (x y z intensity, or x y z rgb with the packed colour in the float's bits).  false: nothing written (an
// empty cloud, with the warning; or a file that cannot be written, with an error).
inline bool SaveBinary(const std::string& filename, const float* rows, size_t n, bool rgb) {
  if (n == 0 || rows == nullptr) {
    std::fprintf(stderr, "[WARNING] Cloud is empty. Do not output to file.\n");
    return false;
  }
  FILE* f = std::fopen(filename.c_str(), "wb");
  if (!f) { std::fprintf(stderr, "[ERROR] cannot write %s\n", filename.c_str()); return false; }
  const std::string h = BinaryHeader(n, rgb);
  bool ok = std::fwrite(h.data(), 1, h.size(), f) == h.size();
  ok = ok && std::fwrite(rows, 4 * sizeof(float), n, f) == n;
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) { std::fprintf(stderr, "[ERROR] short write to %s\n", filename.c_str()); std::remove(filename.c_str()); }
  return ok;
}

}  // namespace pcd
}  // namespace smhip

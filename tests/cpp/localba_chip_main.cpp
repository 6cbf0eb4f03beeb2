// localba_chip_main.cpp -- localba_main.cpp's stand-in keyframes, MapPoints and Map, its scene.bin and
// its out.txt, driving ORB_SLAM2::LocalBundleAdjustmentChipGPU in place of LocalBundleAdjustmentGPU
// (tests/test_localba_chip.py builds it with localba_main.cpp's g++ line).  The stand-ins are not
// copied: the adapter header is included first, then the one call localba_main.cpp makes is renamed
// and its text included.
//
//   localba_chip_main <scene.bin> <out.txt>
#include "cvlite.hpp"
#include "orbslam2_amd/LocalBundleAdjuster.h"

#define LocalBundleAdjustmentGPU LocalBundleAdjustmentChipGPU
#include "localba_main.cpp"

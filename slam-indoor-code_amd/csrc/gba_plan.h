// Global bundle adjustment: the argument check and the observation plan that the device path (gba.hip) and the
// host twin (gba_host.cpp) share.  Plain C++ with no HIP include; defined in gba_host.cpp.
#pragma once

#include "../../include/slamhip.h"

#include <cstdint>
#include <vector>

namespace slamhip {

// The kept observations in camera order and the lists the sums run over (tests/gba_ref.py, "plan").
struct GbaPlan {
    int nk = 0;                         // kept observations
    int behind = 0;                     // excluded with z_c <= zmin at entry
    int points_held = 0, cams_held = 0;
    std::vector<int32_t> cam_off;       // n + 1: camera k owns the kept positions cam_off[k] .. cam_off[k + 1]
    std::vector<int32_t> obs_cam, obs_pt;   // per kept position
    std::vector<double> xy;             // 2 per kept position
    std::vector<int32_t> pt_off, pt_obs;    // m + 1, nk: a point's kept positions, ascending
    std::vector<uint8_t> held;          // n: camera 0 and every camera without a kept observation
};

// SLAM_OK or SLAM_E_INVALID_ARG (include/slamhip.h lists the cases)
int gba_check(const double* K4, const double* cams, int n, const double* points, int m, const int32_t* obs_cam,
              const int32_t* obs_point, const double* obs_xy, int nobs, const slam_gba_params* prm);

// the exclusion rule and the lists; the arguments have passed gba_check
void gba_plan(const double* cams, int n, const double* points, int m, const int32_t* obs_cam, const int32_t* obs_point,
              const double* obs_xy, int nobs, double zmin, GbaPlan& plan);

// the counts of a plan and zeros elsewhere
void gba_summary_init(const GbaPlan& plan, slam_gba_summary* out);

}  // namespace slamhip

// Place recognition: the arithmetic shared by the kernels (place.hip) and the host
// twin (place_host.cpp).  Everything is integer except the one IEEE division of
// the score, so device and host results equal tests/place_ref.py bit for bit.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PLACE_HD __host__ __device__ inline
#else
#define PLACE_HD inline
#endif

namespace slamhip {

enum { kVocSift = 0, kVocOrb = 1 };     // SLAM_VOC_SIFT / SLAM_VOC_ORB
constexpr int kVocMaxWords = 65536;     // 1 <= K <= 2^16
constexpr int kVocMaxDesc = 1 << 24;    // 1 <= N <= 2^24: u32 sums of u8 cannot overflow
constexpr int kBowMaxPerImage = 65535;  // descriptors of one image
constexpr int kBowMaxWeight = 1023;     // idf weights are i32 in [0, 1023]
constexpr int kBowMaxTopk = 32;
constexpr int kVocNoDist = 0x7fffffff;  // the distance of "no centroid seen yet"

// bytes of one descriptor, 0 for an unknown kind
PLACE_HD int voc_desc_bytes(int kind) { return kind == kVocSift ? 128 : kind == kVocOrb ? 32 : 0; }

// (dist, index) order of the top-1: the lower distance, then the lower centroid index
PLACE_HD bool voc_key_lt(int da, int ia, int db, int ib)
{
    return da < db || (da == db && (uint32_t)ia < (uint32_t)ib);
}

// Lloyd update of one SIFT dimension: round-half-up of S / n, n > 0
PLACE_HD uint32_t voc_sift_mean(uint32_t S, uint32_t n)
{
    return (uint32_t)((2ull * S + n) / (2ull * n));
}

// Lloyd update of one ORB bit: the strict majority (a tie gives 0)
PLACE_HD uint32_t voc_orb_bit(uint32_t ones, uint32_t n) { return 2ull * ones > n ? 1u : 0u; }

// one term of the score's numerator: min(a_k B, b_k A), a_k, b_k <= 2^26 and A, B <= 2^26
PLACE_HD int64_t bow_term(uint32_t a, uint64_t A, uint32_t b, uint64_t B)
{
    const int64_t x = (int64_t)((uint64_t)a * B), y = (int64_t)((uint64_t)b * A);
    return x < y ? x : y;
}

// the score from the exact numerator: one IEEE division, 0 when either image is empty
PLACE_HD double bow_score_div(int64_t num, uint64_t A, uint64_t B)
{
    if (A == 0 || B == 0) return 0.0;
    return (double)num / ((double)A * (double)B);
}

// rank order of the top-k: the higher score, then the lower row index
PLACE_HD bool bow_rank_before(double sa, int ia, double sb, int ib)
{
    return sa > sb || (sa == sb && ia < ib);
}

}  // namespace slamhip

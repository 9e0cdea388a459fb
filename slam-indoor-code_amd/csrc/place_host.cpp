// Place recognition on the host: slam_voc_assign_host, slam_voc_train_host,
// slam_bow_vectors_host and slam_bow_score_host, the twins of place.hip's kernels.
// They need no context and no device; the arithmetic is place_math.h's, so the
// results equal the device's and tests/place_ref.py's bit for bit.
#include "../../include/slamhip.h"
#include "place_math.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

namespace slamhip {

int place_check_assign(const void* desc, int n, const void* cent, int K, int kind)
{
    if (voc_desc_bytes(kind) == 0 || n < 0 || n > kVocMaxDesc || K < 1 || K > kVocMaxWords || !cent || (n > 0 && !desc))
        return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

int place_check_train(const void* desc, int n, int K, int iters, int kind, const void* cent, const void* iters_run)
{
    if (voc_desc_bytes(kind) == 0 || n < 1 || n > kVocMaxDesc || K < 1 || K > kVocMaxWords || iters < 0 || !desc ||
        !cent || !iters_run)
        return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

int place_check_vectors(const int32_t* offsets, int m, const int32_t* weights, int K)
{
    if (m < 0 || m > kVocMaxDesc || K < 1 || K > kVocMaxWords || !offsets || !weights) return SLAM_E_INVALID_ARG;
    if (offsets[0] < 0) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < m; i++) {
        const int64_t c = (int64_t)offsets[i + 1] - offsets[i];
        if (c < 0 || c > kBowMaxPerImage) return SLAM_E_INVALID_ARG;
    }
    for (int k = 0; k < K; k++)
        if (weights[k] < 0 || weights[k] > kBowMaxWeight) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

int place_check_score(int nq, int m, int K)
{
    if (nq < 0 || m < 0 || nq > kVocMaxDesc || m > kVocMaxDesc || K < 1 || K > kVocMaxWords) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

int place_check_topk(int nq, int m, int first, int last, int k)
{
    if (nq < 0 || nq > kVocMaxDesc || m < 0 || m > kVocMaxDesc || first < 0 || last < first || last > m || k < 1 ||
        k > kBowMaxTopk)
        return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

namespace {

inline int popc32(uint32_t v) { return __builtin_popcount(v); }

// fn(lo, hi) over [0, n) on up to 16 threads
template <class F> void place_parallel(int n, int grain, F fn)
{
    const int nt = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), (n + grain - 1) / grain}));
    if (nt == 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> pool;
    auto part = [&](int t) { fn((int)((int64_t)n * t / nt), (int)((int64_t)n * (t + 1) / nt)); };
    for (int t = 1; t < nt; t++) pool.emplace_back(part, t);
    part(0);
    for (auto& th : pool) th.join();
}

void assign_rows(const uint8_t* desc, int lo, int hi, const uint8_t* cent, int K, int kind, int32_t* word, int32_t* dist)
{
    const int B = voc_desc_bytes(kind);
    for (int i = lo; i < hi; i++) {
        const uint8_t* x = desc + (size_t)i * B;
        int bd = kVocNoDist, bi = -1;
        for (int c = 0; c < K; c++) {
            const uint8_t* y = cent + (size_t)c * B;
            int d = 0;
            if (kind == kVocSift) {
                for (int j = 0; j < 128; j++) {
                    const int e = (int)x[j] - (int)y[j];
                    d += e * e;
                }
            } else {
                for (int j = 0; j < 32; j++) d += popc32((uint32_t)(x[j] ^ y[j]));
            }
            if (d < bd) {       // strict: a tie keeps the lower centroid index
                bd = d;
                bi = c;
            }
        }
        word[i] = bi;
        dist[i] = bd;
    }
}

void assign_all(const uint8_t* desc, int n, const uint8_t* cent, int K, int kind, int32_t* word, int32_t* dist)
{
    place_parallel(n, 64, [&](int lo, int hi) { assign_rows(desc, lo, hi, cent, K, kind, word, dist); });
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_voc_assign_host(const uint8_t* desc, int n, const uint8_t* cent, int K, int kind, int32_t* word,
                                    int32_t* dist)
{
    if (int rc = place_check_assign(desc, n, cent, K, kind)) return rc;
    if (n == 0) return SLAM_OK;
    if (!word || !dist) return SLAM_E_INVALID_ARG;
    assign_all(desc, n, cent, K, kind, word, dist);
    return SLAM_OK;
}

extern "C" int slam_voc_train_host(const uint8_t* desc, int n, int K, int iters, int kind, uint8_t* cent,
                                   int32_t* iters_run)
{
    if (int rc = place_check_train(desc, n, K, iters, kind, cent, iters_run)) return rc;
    const int B = voc_desc_bytes(kind);
    const int W = kind == kVocSift ? 128 : 256;     // sums per centroid: dimensions or bits
    for (int c = 0; c < K; c++) memcpy(cent + (size_t)c * B, desc + (size_t)((int64_t)c * n / K) * B, B);
    std::vector<int32_t> word((size_t)n), dist((size_t)n);
    std::vector<uint32_t> sum((size_t)K * W), cnt((size_t)K);
    int it = 0;
    while (it < iters) {
        assign_all(desc, n, cent, K, kind, word.data(), dist.data());
        std::fill(sum.begin(), sum.end(), 0u);
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (int i = 0; i < n; i++) {
            const uint8_t* x = desc + (size_t)i * B;
            uint32_t* s = sum.data() + (size_t)word[i] * W;
            cnt[word[i]]++;
            if (kind == kVocSift)
                for (int j = 0; j < 128; j++) s[j] += x[j];
            else
                for (int j = 0; j < 256; j++) s[j] += (x[j >> 3] >> (j & 7)) & 1u;
        }
        bool changed = false;
        for (int c = 0; c < K; c++) {
            if (cnt[c] == 0) continue;      // an empty cluster keeps its centroid
            const uint32_t* s = sum.data() + (size_t)c * W;
            uint8_t nc[128];
            if (kind == kVocSift) {
                for (int j = 0; j < 128; j++) nc[j] = (uint8_t)voc_sift_mean(s[j], cnt[c]);
            } else {
                for (int j = 0; j < 32; j++) {
                    uint32_t v = 0;
                    for (int b = 0; b < 8; b++) v |= voc_orb_bit(s[8 * j + b], cnt[c]) << b;
                    nc[j] = (uint8_t)v;
                }
            }
            if (memcmp(nc, cent + (size_t)c * B, B) != 0) {
                changed = true;
                memcpy(cent + (size_t)c * B, nc, B);
            }
        }
        it++;
        if (!changed) break;
    }
    *iters_run = it;
    return SLAM_OK;
}

extern "C" int slam_bow_vectors_host(const int32_t* word, const int32_t* offsets, int m, const int32_t* weights, int K,
                                     uint32_t* vec, uint64_t* total)
{
    if (int rc = place_check_vectors(offsets, m, weights, K)) return rc;
    if (m == 0) return SLAM_OK;
    if (!vec || !total || (offsets[m] > offsets[0] && !word)) return SLAM_E_INVALID_ARG;
    for (int i = offsets[0]; i < offsets[m]; i++)
        if (word[i] < 0 || word[i] >= K) return SLAM_E_INVALID_ARG;
    for (int r = 0; r < m; r++) {
        uint32_t* v = vec + (size_t)r * K;
        std::fill(v, v + K, 0u);
        for (int i = offsets[r]; i < offsets[r + 1]; i++) v[word[i]]++;
        uint64_t A = 0;
        for (int k = 0; k < K; k++) {
            v[k] *= (uint32_t)weights[k];
            A += v[k];
        }
        total[r] = A;
    }
    return SLAM_OK;
}

extern "C" int slam_bow_score_host(const uint32_t* q, const uint64_t* qtotal, int nq, const uint32_t* db,
                                   const uint64_t* dbtotal, int m, int K, double* scores)
{
    if (int rc = place_check_score(nq, m, K)) return rc;
    if (nq == 0 || m == 0) return SLAM_OK;
    if (!q || !qtotal || !db || !dbtotal || !scores) return SLAM_E_INVALID_ARG;
    place_parallel(m, 16, [&](int lo, int hi) {
        for (int r = lo; r < hi; r++) {
            const uint32_t* b = db + (size_t)r * K;
            const uint64_t Bt = dbtotal[r];
            for (int i = 0; i < nq; i++) {
                const uint32_t* a = q + (size_t)i * K;
                const uint64_t At = qtotal[i];
                uint64_t num = 0;       // unsigned: totals that break the contract wrap instead of overflowing
                if (At != 0 && Bt != 0)
                    for (int k = 0; k < K; k++) num += (uint64_t)bow_term(a[k], At, b[k], Bt);
                scores[(size_t)i * m + r] = bow_score_div((int64_t)num, At, Bt);
            }
        }
    });
    return SLAM_OK;
}

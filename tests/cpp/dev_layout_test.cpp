// Stand-alone check of DevLayout (csrc/dev_layout.h), the planner of every staged
// device buffer: plain C++17, no HIP, built with ASan + UBSan by tests/test_dev_layout.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../slam-indoor-code_amd/csrc/dev_layout.h"

using slamhip::DevLayout;
using slamhip::Slot;

static int checks = 0, failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        checks++;                                                          \
        if (!(cond)) {                                                     \
            failures++;                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                                  \
    } while (0)

struct alignas(32) Wide { double v[4]; };
static_assert(sizeof(Wide) == 32 && alignof(Wide) == 32, "the 32-byte struct of the test");

// the rule of the carve lambdas the layout replaced: offset = running sum of sizes rounded up to 256
static void carve_rule()
{
    const size_t sizes[] = {0, 1, 255, 256, 257, 0, 0, 4096, 3, 512, 1000003, 0, 7};
    DevLayout lay;
    size_t off = 0;
    for (size_t b : sizes) {
        const Slot<uint8_t> s = lay.add_bytes(b);
        CHECK(s.off == off);
        CHECK(s.count == b && s.bytes() == b);
        CHECK(lay.bytes() >= s.end());
        off += (b + 255) & ~(size_t)255;
    }
    CHECK(lay.bytes() == off);
}

template <class T> static void typed(DevLayout& lay, size_t count, size_t& prev_end)
{
    const Slot<T> s = lay.add<T>(count);
    CHECK(s.off % 256 == 0);
    CHECK(s.off % alignof(T) == 0);
    CHECK(s.bytes() == count * sizeof(T));
    CHECK(s.off >= prev_end);               // never overlaps an earlier slot
    CHECK(lay.bytes() >= s.end());
    if (count) prev_end = s.end();
}

static void alignment_and_overlap()
{
    for (size_t count : {(size_t)1, (size_t)3, (size_t)5, (size_t)63, (size_t)257}) {
        DevLayout lay;
        size_t prev_end = 0;
        typed<uint8_t>(lay, count, prev_end);
        typed<int16_t>(lay, count, prev_end);
        typed<int32_t>(lay, count, prev_end);
        typed<float>(lay, count, prev_end);
        typed<double>(lay, count, prev_end);
        typed<uint64_t>(lay, count, prev_end);
        typed<Wide>(lay, count, prev_end);
        typed<uint8_t>(lay, count, prev_end);
        CHECK(lay.bytes() >= prev_end && lay.bytes() < prev_end + 256);
    }
}

static void zero_count()
{
    DevLayout with, without;
    CHECK(with.bytes() == 0);
    const Slot<double> e0 = with.add<double>(0);     // first
    CHECK(e0.off == 0 && e0.bytes() == 0 && with.bytes() == 0);
    const Slot<float> a = with.add<float>(5), a2 = without.add<float>(5);
    const size_t before = with.bytes();
    const Slot<uint64_t> e1 = with.add<uint64_t>(0);     // in the middle
    CHECK(e1.bytes() == 0 && e1.off % 256 == 0 && e1.off >= a.end() && e1.end() <= before && with.bytes() == before);
    const Slot<int32_t> b = with.add<int32_t>(3), b2 = without.add<int32_t>(3);
    const Slot<Wide> e2 = with.add<Wide>(0);           // last
    CHECK(e2.bytes() == 0 && e2.off % 256 == 0 && e2.off >= b.end() && e2.end() <= with.bytes());
    CHECK(a.off == a2.off && b.off == b2.off);
    CHECK(with.bytes() == without.bytes());
    CHECK(with.bytes() >= b.end());
}

static void overflow()
{
    {   // a count whose byte size overflows
        DevLayout lay;
        lay.add<float>(4);
        lay.add<double>(SIZE_MAX / 8 + 1);
        CHECK(lay.bytes() == SIZE_MAX);
        lay.add<uint8_t>(1);                            // stays saturated
        CHECK(lay.bytes() == SIZE_MAX);
        lay.add<uint8_t>(0);
        CHECK(lay.bytes() == SIZE_MAX);
    }
    {   // a sum that overflows
        DevLayout lay;
        lay.add<uint8_t>(SIZE_MAX / 2 + 1);
        CHECK(lay.bytes() == SIZE_MAX / 2 + 1);            // 2^63: already a multiple of 256
        lay.add<uint8_t>(SIZE_MAX / 2 + 1);
        CHECK(lay.bytes() == SIZE_MAX);
    }
    {   // the rounding of a size overflows
        DevLayout lay;
        lay.add<uint8_t>(SIZE_MAX - 100);
        CHECK(lay.bytes() == SIZE_MAX);
    }
    {   // the largest size that still fits does not saturate
        DevLayout lay;
        const Slot<uint8_t> s = lay.add<uint8_t>(SIZE_MAX - 255);
        CHECK(s.off == 0 && lay.bytes() == SIZE_MAX - 255);
        lay.add<uint8_t>(0);
        CHECK(lay.bytes() == SIZE_MAX - 255);
        lay.add<uint8_t>(1);
        CHECK(lay.bytes() == SIZE_MAX);
    }
    {   // a strided slot whose span overflows
        DevLayout lay;
        lay.add_strided(SIZE_MAX / 8, 16, 8);
        CHECK(lay.bytes() == SIZE_MAX);
    }
}

static void strided()
{
    // (n - 1) * stride + 8 bytes: n = 1 at any stride, the packed stride 8, a wider stride
    const size_t cases[][2] = {{1, 8}, {1, 24}, {1, 1 << 20}, {3, 8}, {3, 20}, {1000, 8}, {7, 36}};
    for (const auto& cs : cases) {
        const size_t n = cs[0], stride = cs[1];
        DevLayout lay;
        const Slot<float> head = lay.add<float>(1);
        const Slot<uint8_t> s = lay.add_strided(n, stride, 8);
        CHECK(s.bytes() == (n - 1) * stride + 8);
        CHECK(s.off == 256 && s.off >= head.end());
        CHECK(lay.bytes() >= s.end());
        const Slot<float> next = lay.add<float>(2 * n);
        CHECK(next.off >= s.end() && next.off % 256 == 0);
    }
    DevLayout lay;
    CHECK(lay.add_strided(1, 8, 8).bytes() == 8);
    CHECK(lay.add_strided(5, 8, 8).bytes() == 40);      // stride 8: packed
}

int main()
{
    carve_rule();
    alignment_and_overlap();
    zero_count();
    overflow();
    strided();
    if (failures) {
        std::printf("FAILED: %d of %d checks\n", failures, checks);
        return 1;
    }
    std::printf("OK: %d checks\n", checks);
    return 0;
}

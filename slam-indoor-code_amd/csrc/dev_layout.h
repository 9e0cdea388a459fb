// Layout of one staged device buffer: typed slots carved in order from a
// single allocation.  Plain C++17 with no HIP include: the planning is host
// arithmetic and is unit-tested without a device (tests/cpp/dev_layout_test.cpp).
// The device side (bind, resolve, copy) is DevMem in slamhip_internal.h.
#pragma once

#include <cstddef>
#include <cstdint>

namespace slamhip {

constexpr size_t kSlotAlign = 256;

// count elements of T at byte offset off of the buffer the layout is bound to
template <class T> struct Slot {
    size_t off = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    size_t end() const { return off + bytes(); }
};

// Slots are added in order; each starts at the running end, which is kept
// rounded up to kSlotAlign, so every offset is aligned for any T and bytes()
// covers every slot.  A slot of count 0 is legal and takes no bytes: the next
// slot starts where it would have without it.  Size arithmetic that would
// overflow size_t saturates bytes() to SIZE_MAX, which no allocation satisfies.
class DevLayout {
public:
    template <class T> Slot<T> add(size_t count)
    {
        static_assert(alignof(T) <= kSlotAlign && kSlotAlign % alignof(T) == 0, "a slot's offset is aligned for T");
        if (count > SIZE_MAX / sizeof(T)) return {saturate(), count};
        return {place(count * sizeof(T)), count};
    }
    // raw bytes
    Slot<uint8_t> add_bytes(size_t bytes) { return add<uint8_t>(bytes); }
    // n > 0 elements of elem bytes, one every stride bytes: (n - 1) * stride + elem bytes
    Slot<uint8_t> add_strided(size_t n, size_t stride, size_t elem)
    {
        const size_t gaps = n > 0 ? n - 1 : 0;
        if (stride != 0 && gaps > (SIZE_MAX - elem) / stride) return {saturate(), 0};
        return add_bytes(gaps * stride + elem);
    }
    size_t bytes() const { return end_; }

private:
    size_t saturate() { end_ = SIZE_MAX; return 0; }
    size_t place(size_t b)
    {
        if (end_ == SIZE_MAX || b > SIZE_MAX - (kSlotAlign - 1)) return saturate();
        const size_t off = end_, padded = (b + kSlotAlign - 1) & ~(kSlotAlign - 1);
        if (padded > SIZE_MAX - off) return saturate();
        end_ = off + padded;
        return off;
    }
    size_t end_ = 0;
};

}  // namespace slamhip

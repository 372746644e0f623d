// Two frames as a batch of two at stride cap, the shape every two-frame host entry point hands to its
// batched device call.  Plain host code without a HIP include: a CPU program can compile it.
#pragma once
#include <cstddef>
#include <cstring>

namespace orbx {

// dst[0, 2 * cap): a[0, n1) at dst, b[0, n2) at dst + cap, every other byte fill_byte (0xFF makes the -1 of
// an index table).  A NULL source, whatever its count, is nothing to copy.  n1, n2 <= cap.
template <class T>
void pack_pair(T* dst, size_t cap, const T* a, size_t n1, const T* b, size_t n2, int fill_byte = 0)
{
    if (!a) n1 = 0;
    if (!b) n2 = 0;
    if (n1) std::memcpy(static_cast<void*>(dst), a, sizeof(T) * n1);
    std::memset(static_cast<void*>(dst + n1), fill_byte, sizeof(T) * (cap - n1));
    if (n2) std::memcpy(static_cast<void*>(dst + cap), b, sizeof(T) * n2);
    std::memset(static_cast<void*>(dst + cap + n2), fill_byte, sizeof(T) * (cap - n2));
}

}  // namespace orbx

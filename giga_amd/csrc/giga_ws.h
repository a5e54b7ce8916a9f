// Workspace layout of the geometry stages: a caller's buffer is carved into sub-buffers that each start on a 256-byte boundary.
// A stage describes its workspace once, as a sequence of take<T>(n), and both its *_workspace_bytes and its launcher run that
// description: the size and the offsets cannot drift apart.
#pragma once
#include <cstddef>

namespace giga {

inline size_t ws_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct WsLayout {
    size_t total = 0;
    // offset of the next sub-buffer, n elements of T
    template <typename T>
    size_t take(size_t n) {
        const size_t at = total;
        total += ws_align(n * sizeof(T));
        return at;
    }
};

}  // namespace giga

// The one carver of caller-provided workspaces (host side).  A layout function takes its sub-arrays from a Workspace in a fixed
// order; run over a NULL base it only sizes (every take returns nullptr), so *_workspace_bytes and the call that uses the workspace
// cannot disagree.  Every sub-array starts at a multiple of `align` bytes from the base: 256 for most stages, 16 for the two
// bundle adjustments.  (The renderer's WsLayout, render_common.h, counts in floats and hands offsets to its kernels: another thing.)
#pragma once

#include <cstddef>

class Workspace {
  public:
    Workspace(void* base, size_t align) : base_((char*)base), align_(align) {}

    template <typename T>
    T* take(size_t count) {
        T* p = base_ ? (T*)(base_ + off_) : nullptr;
        off_ += (count * sizeof(T) + align_ - 1) / align_ * align_;
        return p;
    }

    size_t bytes() const { return off_; }       // taken so far, padding included

  private:
    char* base_;
    size_t align_, off_ = 0;
};

// What the translation units of the C ABI share: the struct behind bbfmm_handle, the guard of an entry point, and the
// two device resources that live as long as one call.
#pragma once
#include <cstdint>
#include <memory>
#include <new>
#include <string>

#include "device_group.hpp"
#include "ferreus_bbfmm_hip.h"
#include "fmm_tree.hpp"

struct bbfmm_handle {
    bbfmm::FmmTree tree;                       // the handle's tree; part 0 of its device group when there is one
    std::unique_ptr<bbfmm::DeviceGroup> group; // several devices (or logical parts) behind this one handle
    std::string err;
    int64_t grid_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // of the last bbfmm_evaluate_grid (bbfmm_evaluate_grid_stats)
};

// A failure of the group: its message becomes the handle's.
inline int group_rc(bbfmm_handle *h, int rc) {
    if (rc != BBFMM_OK) h->err = h->group->last_error();
    return rc;
}

namespace bbfmm {

// the message bbfmm_last_error returns for h
inline void set_handle_error(bbfmm_handle *h, const char *message) {
    if (h) h->err = message;
}
inline bool handle_is_host_only(const bbfmm_handle *h) { return h && h->tree.host_only(); }

// Device memory of one call: grows only (what it held is not kept), freed with the call.
template <class T = double>
struct DevBuffer {
    T *p = nullptr;
    int64_t cap = 0;
    DevBuffer() = default;
    DevBuffer(const DevBuffer &) = delete;
    DevBuffer &operator=(const DevBuffer &) = delete;
    ~DevBuffer() { (void)hipFree(p); }
    bool reserve(int64_t n) {
        if (n <= cap) return true;
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
        if (hipMalloc(reinterpret_cast<void **>(&p), static_cast<size_t>(n) * sizeof(T)) != hipSuccess) return false;
        cap = n;
        return true;
    }
};

// A non-blocking stream of the call's own, for the entries that take no handle or a null one.
struct OwnStream {
    hipStream_t st = nullptr;
    OwnStream() = default;
    OwnStream(const OwnStream &) = delete;
    OwnStream &operator=(const OwnStream &) = delete;
    ~OwnStream() {
        if (st) (void)hipStreamDestroy(st);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
};

} // namespace bbfmm

#define GUARD(h)                              \
    if (!(h)) return BBFMM_BAD_ARGUMENT;      \
    try {                                     \
        (h)->err.clear();                     \
        (h)->tree.bind_device();
#define END_GUARD(h)                                   \
    }                                                  \
    catch (const std::bad_alloc &) {                   \
        (h)->err = "out of host memory";               \
        return BBFMM_BAD_ARGUMENT;                     \
    }                                                  \
    catch (const std::exception &e) {                  \
        (h)->err = std::string("exception: ") + e.what(); \
        return BBFMM_BAD_ARGUMENT;                     \
    }                                                  \
    catch (...) {                                      \
        (h)->err = "unknown exception";                \
        return BBFMM_BAD_ARGUMENT;                     \
    }

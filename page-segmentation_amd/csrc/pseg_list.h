// pseg_list.h -- the host scaffold of the list entries and of every other per-device workspace: the device check,
// the workspace table that makes a workspace releasable by existing, the rule that cuts a list into groups, the driver of a list
// call, and the small helpers a group function lays its buffers out with.  Host code only.
#pragma once

#include <mutex>

#include "pseg_common.h"

namespace pseg {

constexpr int PSEG_MAX_DEVICES = 64;                  // entries of every per-device table
// how every list entry cuts its list (include/pseg.h): a group ends after LIST_GROUP_ITEMS items or before LIST_GROUP_BYTES are passed
constexpr int LIST_GROUP_ITEMS = 64;
constexpr size_t LIST_GROUP_BYTES = (size_t)64 << 20;

constexpr size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The device check of every entry that takes a device index; ends with the device current on the calling thread.
inline int open_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(PSEG_EHIP, "no HIP device visible: libpseg has no CPU fallback");
    if (device < 0 || device >= n) return fail(PSEG_EINVAL, "device %d of %d", device, n);
    if (device >= PSEG_MAX_DEVICES) return fail(PSEG_EUNSUPPORTED, "device %d: the per-device tables hold %d devices", device, PSEG_MAX_DEVICES);
    PSEG_HIP(hipSetDevice(device));
    return PSEG_OK;
}

// Every PerDevice of the process, for pseg_release_workspace.  A function-local static: complete before the first constructor
// that registers itself runs, whatever the order of static initialisation, and one instance for all sources of the library.
struct WorkspaceRef { void* self; void (*release)(void* self, int device); };
inline std::vector<WorkspaceRef>& workspace_list() {
    static std::vector<WorkspaceRef> list;
    return list;
}
inline void release_workspaces(int device) {
    for (const WorkspaceRef& w : workspace_list()) w.release(w.self, device);
}

// The one owner of a per-device workspace: one namespace-scope object per workspace type.  Ws is a plain struct of grow-only
// buffers (and a stream or an event where it has one) with a release() that frees them; nothing frees them at process exit.  A
// call locks mu[device] for as long as it uses ws[device].
template <class Ws>
struct PerDevice {
    std::mutex mu[PSEG_MAX_DEVICES];
    Ws ws[PSEG_MAX_DEVICES];
    PerDevice() {
        workspace_list().push_back({this, [](void* self, int device) {
            PerDevice& pd = *(PerDevice*)self;
            std::lock_guard<std::mutex> lk(pd.mu[device]);
            pd.ws[device].release();
        }});
    }
};

// where the group that starts at item g0 ends: LIST_GROUP_ITEMS items, or before LIST_GROUP_BYTES are passed (a single item may pass them)
template <class BytesOf>
int list_group_end(int n, int g0, BytesOf bytes_of) {
    int g1 = g0;
    size_t bytes = 0;
    while (g1 < n && g1 - g0 < LIST_GROUP_ITEMS && (g1 == g0 || bytes + bytes_of(g1) <= LIST_GROUP_BYTES)) {
        bytes += bytes_of(g1);
        ++g1;
    }
    return g1;
}

// A list call on `device`: the device check, the device's lock to the end of the call, `first(ws)` once, then group(ws, g0, g1)
// for every group of the n items.
template <class Ws, class BytesOf, class First, class Group>
int run_list(PerDevice<Ws>& pd, int device, int n, BytesOf bytes_of, First first, Group group) {
    PSEG_TRY(open_device(device));
    std::lock_guard<std::mutex> lk(pd.mu[device]);
    Ws& ws = pd.ws[device];
    PSEG_TRY(first(ws));
    for (int g0 = 0; g0 < n;) {
        const int g1 = list_group_end(n, g0, bytes_of);
        PSEG_TRY(group(ws, g0, g1));
        g0 = g1;
    }
    return PSEG_OK;
}
template <class Ws, class BytesOf, class Group>
int run_list(PerDevice<Ws>& pd, int device, int n, BytesOf bytes_of, Group group) {
    return run_list(pd, device, n, bytes_of, [](Ws&) { return (int)PSEG_OK; }, group);
}

// An error return in the middle of a group leaves no copy from / to the caller's arrays in flight: every way out waits for the
// group's stream, except the normal one, which disarms the drain after its own wait.
struct GroupDrain {
    hipStream_t st;
    bool armed = true;
    ~GroupDrain() { if (armed) (void)hipStreamSynchronize(st); }
};

// Byte offsets of buffers laid out one behind the other: take() returns where the next one starts and moves on by its size,
// rounded up to `align`.
struct Bump {
    size_t off = 0;
    size_t take(size_t bytes, size_t align = 256) {
        const size_t at = off;
        off += (bytes + align - 1) / align * align;
        return at;
    }
};

}  // namespace pseg

// Device ops: HBM-resident snapshot engine on the gfx950 kernels in
// cpp/hip/snapshot_kernels.hip (dirty-page tracking, compacted XOR diff,
// merge application, elementwise reductions).
//
// This is the MI355X-native replacement for the reference's fault-driven
// dirty tracking + CPU diff loops (reference: src/util/dirty.cpp,
// src/util/snapshot.cpp:30-652): there is no mprotect on HBM, so dirty
// pages come from a compare kernel against the snapshot baseline, and the
// XOR page diff IS the shippable delta (DIFFING_MODE=xor made native).
#pragma once

#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "faabricamd/snapshot.h"

namespace faabricamd {

bool gpuAvailable();
int gpuCount();

// Raw kernel entry points (extern "C" in the .hip TU)
extern "C" {
hipError_t famDirtyPages(const void* snap,
                         const void* cur,
                         uint64_t bytes,
                         uint32_t* flagsDev,
                         hipStream_t stream);
// NT device-to-device copy (beats hipMemcpy D2D for large HBM buffers)
hipError_t famCopyBuffer(const void* src,
                         void* dst,
                         uint64_t bytes,
                         hipStream_t stream);
// Deterministic pseudo-random fill / scattered page mutation (bench
// init for the random-byte snapshot shapes, BASELINE.json config 4)
hipError_t famFillRandom(void* buf,
                         uint64_t bytes,
                         uint64_t seed,
                         hipStream_t stream);
hipError_t famTouchPages(void* buf,
                         const uint32_t* pagesDev,
                         uint32_t nPages,
                         uint64_t seed,
                         hipStream_t stream);

hipError_t famXorBuffer(const void* a,
                        const void* b,
                        void* out,
                        uint64_t bytes,
                        hipStream_t stream);
hipError_t famDiffXorPages(const void* snap,
                           const void* cur,
                           uint64_t bytes,
                           uint32_t* ticketDev,
                           uint32_t* pageIdxDev,
                           void* payloadDev,
                           uint32_t* bitmapDev,
                           hipStream_t stream);
hipError_t famApplyXorPages(void* snap,
                            const uint32_t* pageIdxDev,
                            const void* payloadDev,
                            uint32_t nDirty,
                            hipStream_t stream);
hipError_t famApplyXorPagesEx(void* snap,
                              const uint32_t* pageIdxDev,
                              const void* payloadDev,
                              uint32_t nDirty,
                              int compact,
                              hipStream_t stream);
hipError_t famGatherPages(const void* payloadDev,
                          const uint32_t* pageIdxDev,
                          void* outDev,
                          uint32_t nDirty,
                          hipStream_t stream);
// State-KV mirror commit (famKvCommitPagesKernel): copy the listed 4 KiB
// pages of a pinned host mirror to the same offsets of the HBM value,
// one block per page. srcHostMapped and pageIdx are device-visible
// pointers to pinned host memory (hipHostGetDevicePointer); the value's
// partial last page is copied to the byte.
hipError_t famCommitPages(const void* srcHostMapped,
                          void* dstDev,
                          const uint32_t* pageIdx,
                          uint32_t nPages,
                          uint64_t valueBytes,
                          hipStream_t stream);
hipError_t famElementwiseOp(void* inout,
                            const void* in,
                            uint64_t count,
                            int dtype,
                            int op,
                            hipStream_t stream);
// Typed merge regions. dtype is a SnapshotDataType code (Int, Long, Float,
// Double) and op a SnapshotMergeOperation code (Sum, Product, Subtract,
// Max, Min); anything else is hipErrorInvalidValue.
//
// famTypedDiff (typedDiffKernel): compacted typed diff of nElems elements
// at byte regionStart (a multiple of the element size) of cur against
// snap, both 16 B-aligned. An element is changed when !(orig == cur);
// each changed one appends {index relative to the region start, value} to
// idxOutDev/valOutDev (room for nElems entries, order unspecified), where
// value is cur - orig (Sum), orig - cur (Subtract), cur / orig (Product)
// or cur (Max, Min). *ticketDev and *errDev are zeroed by the caller:
// afterwards the ticket is the entry count and the error word is non-zero
// if a changed Product element had a zero original (nothing is emitted
// for it).
hipError_t famTypedDiff(const void* snap,
                        const void* cur,
                        uint64_t regionStart,
                        uint64_t nElems,
                        int dtype,
                        int op,
                        uint32_t* ticketDev,
                        uint32_t* errDev,
                        uint32_t* idxOutDev,
                        void* valOutDev,
                        hipStream_t stream);
// famApplyTypedElems (applyTypedElemsKernel): base[idx[i]] =
// op(base[idx[i]], val[i]) for i < count, base being the region start.
// Max/Min keep std::max/std::min(target, value) operand order. The caller
// has checked every index; count == 0 launches nothing.
hipError_t famApplyTypedElems(void* base,
                              const uint32_t* idxDev,
                              const void* valDev,
                              uint32_t count,
                              int dtype,
                              int op,
                              hipStream_t stream);
}

inline constexpr size_t DEVICE_PAGE = 4096;

// An HBM-resident snapshot of a device memory region, with the
// diff/merge pipeline. All methods are synchronous on the owned stream.
class DeviceSnapshot
{
  public:
    // device -1 = this worker's configured GPU (FAABRIC_GPU_DEVICE)
    DeviceSnapshot(size_t bytes, int device = -1);
    ~DeviceSnapshot();
    DeviceSnapshot(const DeviceSnapshot&) = delete;

    size_t size() const { return bytes_; }
    int device() const { return device_; }
    void* data() { return snap_; }

    // Baseline management
    void copyInHost(const void* hostBuf, size_t n, size_t offset = 0);
    void copyOutHost(void* hostBuf, size_t n, size_t offset = 0) const;
    void captureFromDevice(const void* devPtr); // snapshot := memory view

    // Dirty-page bitmap of devPtr vs the snapshot (one u32 flag per 4 KiB
    // page, copied back to the host)
    std::vector<uint32_t> dirtyPages(const void* devPtr);

    // Compacted XOR page diff of devPtr vs the snapshot. Returns the
    // number of dirty pages; the page indices + payload stay on-device
    // (diffPageIdx()/diffPayload()) ready to ship or apply.
    uint32_t diffXor(const void* devPtr);

    // Merge: snapshot ^= last diff (applies the compacted pages)
    void applyLastDiff();
    // Merge a diff produced elsewhere (e.g. shipped from a peer GPU)
    void applyDiffPages(const uint32_t* pageIdxDev,
                        const void* payloadDev,
                        uint32_t nDirty);

    // Ship/receive the compact wire form: {page indices, slot-compacted
    // 4 KiB payloads}
    void gatherLastDiffToHost(std::vector<uint32_t>& pagesOut,
                              std::vector<uint8_t>& payloadOut);
    void applyCompactDiffFromHost(const std::vector<uint32_t>& pages,
                                  const uint8_t* payload,
                                  size_t payloadBytes);

    // --- typed merge regions (Sum/Subtract/Product/Max/Min over
    // Int/Long/Float/Double; see SnapshotMergeOperation::TypedElems) ---
    // These three methods may be called from several threads on one
    // snapshot: they take one lock between them. The page-diff methods
    // above (diffXor, gatherLastDiffToHost, applyLastDiff, ...) keep their
    // unlocked shared scratch, so a caller must not run those, or the
    // join-time queue drain, concurrently with anything else on the
    // same snapshot.

    // Typed diff of one region of devPtr vs the snapshot, as the packed
    // TypedElems diff; nothing when no element changed. The region ends at
    // offset + length, or at the snapshot's end when length == 0; trailing
    // bytes that do not fill an element are not diffed. Throws on a
    // Product element with a zero original.
    std::optional<SnapshotDiff> typedDiff(const void* devPtr,
                                          const SnapshotMergeRegion& region);
    // Validate (validateTypedElemsDiff), upload and merge a TypedElems
    // diff into the snapshot
    void applyTypedDiff(const SnapshotDiff& diff);
    // The full thread diff of devPtr vs the snapshot under merge regions:
    // one TypedElems diff per typed region that changed, plus one XorPages
    // diff for everything else (typed bytes zeroed in its payload, pages
    // wholly inside typed regions dropped). Leaves the filtered page list
    // as the last diff.
    std::vector<SnapshotDiff> diffWithRegions(
      const void* devPtr,
      const std::vector<SnapshotMergeRegion>& regions);

    // Queued XorPages / TypedElems diffs from remote/other-thread merges,
    // applied in arrival order at join time. queuePackedDiff takes the
    // XorPages wire form ([u32 n][u32 pages[n]][n*4KiB]) bare.
    void queueDiff(SnapshotDiff diff);
    void queuePackedDiff(std::vector<uint8_t> packed);
    int applyQueuedPackedDiffs();

    const uint32_t* diffPageIdx() const { return pageIdx_; }
    const void* diffPayload() const { return payload_; }
    uint32_t lastDiffPages() const { return lastDirty_; }
    hipStream_t stream() const { return stream_; }

  private:
    void ensureDiffBuffers();
    void ensureTypedScratch(size_t count, size_t elemSize);

    size_t bytes_ = 0;
    int device_ = 0;
    uint8_t* snap_ = nullptr;
    hipStream_t stream_ = nullptr;

    // Diff scratch (lazily allocated): worst case every page dirty.
    // The payload buffer is SPARSE (indexed by page); pageIdx_ is the
    // compacted dirty list.
    uint32_t* ticket_ = nullptr;
    uint32_t* pageIdx_ = nullptr;
    uint8_t* payload_ = nullptr;
    uint32_t* bitmap_ = nullptr;
    uint32_t lastDirty_ = 0;

    // Typed diff/apply scratch, grown to the largest region seen:
    // {ticket, error word}, element indices, values
    uint32_t* typedCtl_ = nullptr;
    uint32_t* typedIdx_ = nullptr;
    uint8_t* typedVal_ = nullptr;
    size_t typedIdxCap_ = 0;
    size_t typedValCap_ = 0;
    // typedDiff, applyTypedDiff and diffWithRegions share this scratch and
    // the stream: they serialise on one (recursive) lock
    std::recursive_mutex typedMx_;

    std::mutex queueMx_;
    std::vector<SnapshotDiff> queued_;
};

// Check the merge regions of a THREADS fork over a device arena of
// arenaSize bytes and return the typed ones sorted by offset. A typed op
// (Sum..Min) needs a typed element type, an element-aligned offset inside
// the arena and no overlap with another typed region; Bytewise and XOR
// over Raw mean default XOR paging. Anything else throws.
std::vector<SnapshotMergeRegion> validateDeviceMergeRegions(
  const std::vector<SnapshotMergeRegion>& regions,
  size_t arenaSize);

// Registry of HBM-resident snapshots (device analog of SnapshotRegistry)
class DeviceSnapshotRegistry
{
  public:
    static DeviceSnapshotRegistry& get();
    std::shared_ptr<DeviceSnapshot> getSnapshot(const std::string& key);
    bool snapshotExists(const std::string& key);
    void registerSnapshot(const std::string& key,
                          std::shared_ptr<DeviceSnapshot> snap);
    void deleteSnapshot(const std::string& key);
    void clear();

    // Merge regions of a fork travel by key, not on the snapshot object
    // (an empty list erases; none set reads as empty)
    void setMergeRegions(const std::string& key,
                         const std::vector<SnapshotMergeRegion>& regions);
    std::vector<SnapshotMergeRegion> getMergeRegions(const std::string& key);

  private:
    std::mutex mx;
    std::map<std::string, std::shared_ptr<DeviceSnapshot>> snapshots;
    std::map<std::string, std::vector<SnapshotMergeRegion>> mergeRegions;
};

// Elementwise op on device buffers: inout = op(inout, in)
// dtype matches MpiDataType; op matches MpiOp (+4=sub, 5=xor)
void deviceElementwiseOp(void* inout,
                         const void* in,
                         uint64_t count,
                         int dtype,
                         int op,
                         hipStream_t stream = nullptr);

} // namespace faabricamd

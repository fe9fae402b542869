// Snapshots: registry, merge regions, typed diffs, restore.
//
// MI355X-native re-design of the reference snapshot subsystem
// (reference: include/faabric/util/snapshot.h:21-341,
//  src/util/snapshot.cpp:30-652, snapshot/SnapshotRegistry.h:13-41,
//  src/snapshot/SnapshotServer.cpp:28-62, snapshot/SnapshotClient.h:40-62).
// Differences by design:
//  - a SnapshotData may be HOST-resident (std::vector arena; mmap/memfd in
//    the reference) or DEVICE-resident in MI355X HBM3E; diff/apply over
//    device memory run as hand-written gfx950 HIP kernels (cpp/hip/)
//  - diffs are computed by comparing against the snapshot (the reference's
//    "xor"-style diffing, DIFFING_MODE=xor src/util/config.cpp:82) — there
//    is no mprotect/userfaultfd on HBM, so fault-driven tracking is
//    replaced by a page-bitmap compare kernel
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "faabricamd/messages.h"
#include "faabricamd/transport.h"

namespace faabricamd {

inline constexpr size_t SNAPSHOT_PAGE_SIZE = 4096;
// Byte-diff compare granularity (reference: util/snapshot.h:21
// ARRAY_COMP_CHUNK_SIZE = 128)
inline constexpr size_t DIFF_CHUNK_SIZE = 128;

enum class SnapshotDataType : int32_t
{
    Raw = 0,
    Bool = 1,
    Int = 2,
    Long = 3,
    Float = 4,
    Double = 5,
};

enum class SnapshotMergeOperation : int32_t
{
    Bytewise = 0,
    Sum = 1,
    Product = 2,
    Subtract = 3,
    Max = 4,
    Min = 5,
    XOR = 6,
    // Packed page form used by the GPU THREADS flow (this project's own
    // extension): data = [u32 n][u32 pageIdx[n]][n x 4 KiB XOR payloads]
    XorPages = 7,
    // Packed element form of a typed merge region on the GPU THREADS flow
    // (this project's own extension): dataType = element type, offset =
    // the region's byte offset, data = [u32 op][u32 count]
    // [u32 elemIdx[count]][zero pad to 8 B][T value[count]], little-endian,
    // where op is the real merge operation (Sum..Min)
    TypedElems = 8,
};

struct SnapshotDiff
{
    SnapshotDiff() = default;
    SnapshotDiff(SnapshotDataType dataTypeIn,
                 SnapshotMergeOperation operationIn,
                 uint32_t offsetIn,
                 const uint8_t* data,
                 size_t size)
      : dataType(dataTypeIn)
      , operation(operationIn)
      , offset(offsetIn)
      , dataCopy(data, data + size)
    {}

    SnapshotDataType dataType = SnapshotDataType::Raw;
    SnapshotMergeOperation operation = SnapshotMergeOperation::Bytewise;
    uint32_t offset = 0;
    std::vector<uint8_t> dataCopy;

    const uint8_t* getData() const { return dataCopy.data(); }
    size_t size() const { return dataCopy.size(); }

    SnapshotDiffMsg toMsg() const;
    static SnapshotDiff fromMsg(const SnapshotDiffMsg& msg);
};

// sizeof(T) of a typed-merge element type (Int, Long, Float, Double), 0 for
// the others
size_t snapshotTypedElemSize(SnapshotDataType dataType);
bool isTypedMergeOperation(SnapshotMergeOperation op);

// A validated view into a TypedElems diff's data
struct TypedElemsView
{
    SnapshotMergeOperation op = SnapshotMergeOperation::Sum;
    uint32_t count = 0;
    size_t elemSize = 0;
    const uint8_t* idx = nullptr;    // count x u32
    const uint8_t* values = nullptr; // count x elemSize, 8 B-aligned offset
};

size_t typedElemsPackedSize(uint32_t count, size_t elemSize);

// The one validator of the TypedElems wire form, run by every consumer
// before anything is uploaded or applied: exact size for the count, a
// typed op and element type, an element-aligned offset and every element
// inside snapshotSize. Throws FaabricException on a violation.
TypedElemsView validateTypedElemsDiff(const SnapshotDiff& diff,
                                      size_t snapshotSize);

struct SnapshotMergeRegion
{
    SnapshotMergeRegion() = default;
    SnapshotMergeRegion(uint32_t offsetIn,
                        size_t lengthIn,
                        SnapshotDataType dataTypeIn,
                        SnapshotMergeOperation operationIn)
      : offset(offsetIn)
      , length(lengthIn)
      , dataType(dataTypeIn)
      , operation(operationIn)
    {}

    uint32_t offset = 0;
    size_t length = 0;
    SnapshotDataType dataType = SnapshotDataType::Raw;
    SnapshotMergeOperation operation = SnapshotMergeOperation::Bytewise;

    // Per-region typed diff calculation over the dirty pages
    // (reference: src/util/snapshot.cpp:652 addDiffs)
    void addDiffs(std::vector<SnapshotDiff>& diffs,
                  const uint8_t* original,
                  size_t originalSize,
                  const uint8_t* updated,
                  size_t updatedSize,
                  const std::vector<char>& dirtyPages) const;
};

// Byte-level diff of [startOffset, endOffset) in DIFF_CHUNK_SIZE chunks with
// byte refinement (reference: src/util/snapshot.cpp:30 diffArrayRegions)
void diffArrayRegions(std::vector<SnapshotDiff>& diffs,
                      uint32_t startOffset,
                      uint32_t endOffset,
                      const uint8_t* original,
                      const uint8_t* updated);

class SnapshotData
{
  public:
    SnapshotData() = default;
    explicit SnapshotData(size_t sizeIn);
    SnapshotData(size_t sizeIn, size_t maxSizeIn);
    explicit SnapshotData(const std::vector<uint8_t>& dataIn);
    SnapshotData(const std::vector<uint8_t>& dataIn, size_t maxSizeIn);
    ~SnapshotData();

    SnapshotData(const SnapshotData&) = delete;
    SnapshotData& operator=(const SnapshotData&) = delete;

    size_t getSize() const { return size_; }
    size_t getMaxSize() const { return maxSize_; }

    uint8_t* getMutableDataPtr(size_t offset = 0);
    const uint8_t* getDataPtr(size_t offset = 0) const;
    std::vector<uint8_t> getDataCopy() const;
    std::vector<uint8_t> getDataCopy(uint32_t offset, size_t size) const;

    void copyInData(const std::vector<uint8_t>& buffer, uint32_t offset = 0);
    void copyInData(const uint8_t* buffer, size_t size, uint32_t offset);

    // Restore: copy the snapshot over a memory view
    // (reference: mapToMemory src/util/snapshot.cpp:326)
    void mapToMemory(uint8_t* target, size_t targetSize) const;

    // --- merge regions ---
    void addMergeRegion(uint32_t offset,
                        size_t length,
                        SnapshotDataType dataType,
                        SnapshotMergeOperation operation);
    void fillGapsWithBytewiseRegions();
    void clearMergeRegions();
    std::map<uint32_t, SnapshotMergeRegion> getMergeRegions();

    // --- diffing ---
    std::vector<SnapshotDiff> diffWithDirtyRegions(
      const uint8_t* updated,
      size_t updatedSize,
      const std::vector<char>& dirtyPages);
    // Compare-everything convenience (dirtyPages = all)
    std::vector<SnapshotDiff> diffWithMemory(const uint8_t* updated,
                                             size_t updatedSize);

    // --- applying diffs (typed merges) ---
    void applyDiff(const SnapshotDiff& diff);
    void applyDiffs(const std::vector<SnapshotDiff>& diffs);
    void queueDiffs(const std::vector<SnapshotDiff>& diffs);
    int writeQueuedDiffs();

    // Grow to the given size (zero-filled)
    void setSnapshotSize(size_t newSize);

  private:
    size_t size_ = 0;
    size_t maxSize_ = 0;
    std::vector<uint8_t> data_;

    std::mutex snapMx;
    std::map<uint32_t, SnapshotMergeRegion> mergeRegions;
    std::vector<SnapshotDiff> queuedDiffs;
};

// ------------------------- registry -----------------------------------------

class SnapshotRegistry
{
  public:
    static SnapshotRegistry& get();

    std::shared_ptr<SnapshotData> getSnapshot(const std::string& key);
    bool snapshotExists(const std::string& key);
    void registerSnapshot(const std::string& key,
                          std::shared_ptr<SnapshotData> data);
    void registerSnapshotIfNotExists(const std::string& key,
                                     std::shared_ptr<SnapshotData> data);
    void deleteSnapshot(const std::string& key);
    size_t getSnapshotCount();
    void clear();

  private:
    std::mutex mx;
    std::map<std::string, std::shared_ptr<SnapshotData>> snapshots;
};

// ------------------------- RPC ----------------------------------------------

// (reference: snapshot/SnapshotApi.h:4-11)
enum class SnapshotCalls : uint8_t
{
    PushSnapshot = 1,
    PushSnapshotUpdate = 2,
    DeleteSnapshot = 3,
    ThreadResult = 4,
    // Chunk of a device snapshot shipped via HIP IPC (same-node workers):
    // payload is already in our arena, body is an IpcChunk
    PushSnapshotIpc = 5,
    // Device (HBM) snapshot as host bytes — our extension beyond the
    // reference's flatbuffers surface, so it rides its own call
    PushSnapshotDevice = 6,
    // Merge regions of a device snapshot, stored by key (the IPC landing
    // path creates the snapshot object on its first chunk, so the object
    // cannot carry them): body is a SnapshotPushRequest with no contents
    DeviceMergeRegions = 7,
};

class SnapshotServer : public MessageEndpointServer
{
  public:
    SnapshotServer();
    void doAsyncRecv(uint8_t code,
                     const std::string& body,
                     uint32_t seq) override;
    std::string doSyncRecv(uint8_t code, const std::string& body) override;
};

class SnapshotClient : public MessageEndpointClient
{
  public:
    explicit SnapshotClient(const std::string& host);
    void pushSnapshot(const std::string& key, SnapshotData& data);
    // HBM-resident snapshot: ships the contents and re-registers them in
    // the destination's device registry
    void pushDeviceSnapshot(const std::string& key, const void* hostCopy,
                            size_t size);
    // Same, straight from HBM: same-node workers stream arena chunks
    // over xGMI (no D2H); falls back to a host copy + pushDeviceSnapshot
    void pushDeviceSnapshotFromDevice(const std::string& key,
                                      const void* devPtr,
                                      size_t size);
    // Sent before the device snapshot itself, so a remote thread that
    // waited for the snapshot finds its regions
    void pushDeviceMergeRegions(
      const std::string& key,
      const std::vector<SnapshotMergeRegion>& regions);
    void pushSnapshotUpdate(const std::string& key,
                            const std::vector<SnapshotDiff>& diffs,
                            const std::vector<SnapshotMergeRegion>& regions);
    void pushThreadResult(int32_t appId,
                          int32_t messageId,
                          int32_t returnValue,
                          const std::string& key,
                          const std::vector<SnapshotDiff>& diffs);
    void deleteSnapshot(const std::string& key);
};

std::shared_ptr<SnapshotClient> getSnapshotClient(const std::string& host);
void clearSnapshotClients();

// Mock-mode recording (reference: snapshot/SnapshotClient.h:13-36)
std::vector<std::pair<std::string, std::string>> getSnapshotPushesMock();
std::vector<std::pair<std::string, ThreadResultRequest>>
getThreadResultsMock();
void clearMockedSnapshotRequests();

} // namespace faabricamd

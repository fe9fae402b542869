// Device snapshot engine host-side wrappers (kernels:
// cpp/hip/snapshot_kernels.hip). Fails loudly when no GPU is present —
// the CPU path lives in snapshot.cpp, never silently substituted here.
#include "faabricamd/ops.h"
#include "faabricamd/util.h"

#include <algorithm>
#include <cstring>

namespace faabricamd {

#define OPS_HIP_CHECK(call)                                                    \
    do {                                                                       \
        hipError_t err_ = (call);                                              \
        if (err_ != hipSuccess) {                                              \
            throw FaabricException(std::string("HIP error in ops: ") +         \
                                   hipGetErrorString(err_));                   \
        }                                                                      \
    } while (0)

bool gpuAvailable()
{
    return gpuCount() > 0;
}

int gpuCount()
{
    static int n = []() {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) {
            return 0;
        }
        return count;
    }();
    return n;
}

DeviceSnapshot::DeviceSnapshot(size_t bytes, int device)
  : bytes_(bytes)
  , device_(device)
{
    if (device_ < 0) {
        device_ = getSystemConfig().gpuDevice;
    }
    if ((bytes % DEVICE_PAGE) != 0) {
        throw FaabricException("device snapshot size must be page-aligned");
    }
    if (!gpuAvailable()) {
        throw FaabricException(
          "DeviceSnapshot requires an MI355X GPU (none visible)");
    }
    OPS_HIP_CHECK(hipSetDevice(device_));
    OPS_HIP_CHECK(hipMalloc(&snap_, bytes_));
    OPS_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
}

DeviceSnapshot::~DeviceSnapshot()
{
    if (snap_ != nullptr) {
        hipFree(snap_);
    }
    if (ticket_ != nullptr) {
        hipFree(ticket_);
    }
    if (pageIdx_ != nullptr) {
        hipFree(pageIdx_);
    }
    if (payload_ != nullptr) {
        hipFree(payload_);
    }
    if (bitmap_ != nullptr) {
        hipFree(bitmap_);
    }
    if (typedCtl_ != nullptr) {
        hipFree(typedCtl_);
    }
    if (typedIdx_ != nullptr) {
        hipFree(typedIdx_);
    }
    if (typedVal_ != nullptr) {
        hipFree(typedVal_);
    }
    if (stream_ != nullptr) {
        hipStreamDestroy(stream_);
    }
}

void DeviceSnapshot::copyInHost(const void* hostBuf, size_t n, size_t offset)
{
    OPS_HIP_CHECK(hipSetDevice(device_));
    OPS_HIP_CHECK(hipMemcpyAsync(
      snap_ + offset, hostBuf, n, hipMemcpyHostToDevice, stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSnapshot::copyOutHost(void* hostBuf, size_t n, size_t offset) const
{
    OPS_HIP_CHECK(hipSetDevice(device_));
    OPS_HIP_CHECK(hipMemcpyAsync(
      hostBuf, snap_ + offset, n, hipMemcpyDeviceToHost, stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSnapshot::captureFromDevice(const void* devPtr)
{
    OPS_HIP_CHECK(hipSetDevice(device_));
    OPS_HIP_CHECK(hipMemcpyAsync(
      snap_, devPtr, bytes_, hipMemcpyDeviceToDevice, stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSnapshot::ensureDiffBuffers()
{
    if (ticket_ != nullptr) {
        return;
    }
    size_t nPages = bytes_ / DEVICE_PAGE;
    OPS_HIP_CHECK(hipMalloc(&ticket_, sizeof(uint32_t)));
    OPS_HIP_CHECK(hipMalloc(&pageIdx_, nPages * sizeof(uint32_t)));
    OPS_HIP_CHECK(hipMalloc(&payload_, bytes_));
    OPS_HIP_CHECK(hipMalloc(&bitmap_, ((nPages + 31) / 32) * sizeof(uint32_t)));
}

std::vector<uint32_t> DeviceSnapshot::dirtyPages(const void* devPtr)
{
    OPS_HIP_CHECK(hipSetDevice(device_));
    size_t nPages = bytes_ / DEVICE_PAGE;
    uint32_t* flagsDev = nullptr;
    OPS_HIP_CHECK(hipMalloc(&flagsDev, nPages * sizeof(uint32_t)));
    OPS_HIP_CHECK(
      hipMemsetAsync(flagsDev, 0, nPages * sizeof(uint32_t), stream_));
    OPS_HIP_CHECK(famDirtyPages(snap_, devPtr, bytes_, flagsDev, stream_));
    std::vector<uint32_t> flags(nPages);
    OPS_HIP_CHECK(hipMemcpyAsync(flags.data(),
                                 flagsDev,
                                 nPages * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost,
                                 stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
    hipFree(flagsDev);
    return flags;
}

uint32_t DeviceSnapshot::diffXor(const void* devPtr)
{
    OPS_HIP_CHECK(hipSetDevice(device_));
    ensureDiffBuffers();
    size_t nWords = (bytes_ / DEVICE_PAGE + 31) / 32;
    OPS_HIP_CHECK(hipMemsetAsync(ticket_, 0, sizeof(uint32_t), stream_));
    OPS_HIP_CHECK(
      hipMemsetAsync(bitmap_, 0, nWords * sizeof(uint32_t), stream_));
    OPS_HIP_CHECK(famDiffXorPages(snap_, devPtr, bytes_, ticket_, pageIdx_,
                                  payload_, bitmap_, stream_));
    uint32_t nDirty = 0;
    OPS_HIP_CHECK(hipMemcpyAsync(&nDirty,
                                 ticket_,
                                 sizeof(uint32_t),
                                 hipMemcpyDeviceToHost,
                                 stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
    lastDirty_ = nDirty;
    return nDirty;
}

void DeviceSnapshot::applyLastDiff()
{
    applyDiffPages(pageIdx_, payload_, lastDirty_);
}

void DeviceSnapshot::applyDiffPages(const uint32_t* pageIdxDev,
                                    const void* payloadDev,
                                    uint32_t nDirty)
{
    if (nDirty == 0) {
        return;
    }
    OPS_HIP_CHECK(hipSetDevice(device_));
    OPS_HIP_CHECK(
      famApplyXorPages(snap_, pageIdxDev, payloadDev, nDirty, stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
}

void DeviceSnapshot::gatherLastDiffToHost(std::vector<uint32_t>& pagesOut,
                                          std::vector<uint8_t>& payloadOut)
{
    OPS_HIP_CHECK(hipSetDevice(device_));
    pagesOut.resize(lastDirty_);
    payloadOut.resize((size_t)lastDirty_ * DEVICE_PAGE);
    if (lastDirty_ == 0) {
        return;
    }
    // Gather on-device, then one contiguous D2H copy
    uint8_t* compactDev = nullptr;
    OPS_HIP_CHECK(
      hipMalloc(&compactDev, (size_t)lastDirty_ * DEVICE_PAGE));
    OPS_HIP_CHECK(
      famGatherPages(payload_, pageIdx_, compactDev, lastDirty_, stream_));
    OPS_HIP_CHECK(hipMemcpyAsync(pagesOut.data(),
                                 pageIdx_,
                                 lastDirty_ * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost,
                                 stream_));
    OPS_HIP_CHECK(hipMemcpyAsync(payloadOut.data(),
                                 compactDev,
                                 (size_t)lastDirty_ * DEVICE_PAGE,
                                 hipMemcpyDeviceToHost,
                                 stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
    hipFree(compactDev);
}

void DeviceSnapshot::applyCompactDiffFromHost(
  const std::vector<uint32_t>& pages,
  const uint8_t* payload,
  size_t payloadBytes)
{
    if (pages.empty()) {
        return;
    }
    if (payloadBytes != pages.size() * DEVICE_PAGE) {
        throw FaabricException("compact diff size mismatch");
    }
    // Page indices come off the wire; an out-of-range index would make
    // the XOR kernel write past the snapshot allocation in HBM.
    const size_t nPages = (bytes_ + DEVICE_PAGE - 1) / DEVICE_PAGE;
    for (uint32_t p : pages) {
        if ((size_t)p >= nPages) {
            throw FaabricException("compact diff page out of range");
        }
    }
    OPS_HIP_CHECK(hipSetDevice(device_));
    uint32_t* pagesDev = nullptr;
    uint8_t* payloadDev = nullptr;
    OPS_HIP_CHECK(hipMalloc(&pagesDev, pages.size() * sizeof(uint32_t)));
    OPS_HIP_CHECK(hipMalloc(&payloadDev, payloadBytes));
    OPS_HIP_CHECK(hipMemcpyAsync(pagesDev,
                                 pages.data(),
                                 pages.size() * sizeof(uint32_t),
                                 hipMemcpyHostToDevice,
                                 stream_));
    OPS_HIP_CHECK(hipMemcpyAsync(payloadDev,
                                 payload,
                                 payloadBytes,
                                 hipMemcpyHostToDevice,
                                 stream_));
    OPS_HIP_CHECK(famApplyXorPagesEx(snap_,
                                     pagesDev,
                                     payloadDev,
                                     (uint32_t)pages.size(),
                                     /*compact=*/1,
                                     stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
    hipFree(pagesDev);
    hipFree(payloadDev);
}

// ------------------------- typed merge regions -------------------------------

std::vector<SnapshotMergeRegion> validateDeviceMergeRegions(
  const std::vector<SnapshotMergeRegion>& regions,
  size_t arenaSize)
{
    std::vector<SnapshotMergeRegion> typed;
    for (const auto& r : regions) {
        if (r.operation == SnapshotMergeOperation::Bytewise ||
            r.operation == SnapshotMergeOperation::XOR) {
            if (r.dataType != SnapshotDataType::Raw) {
                throw FaabricException(
                  "device merge region: Bytewise/XOR need the Raw type");
            }
            continue; // default XOR paging
        }
        if (!isTypedMergeOperation(r.operation)) {
            throw FaabricException(
              "device merge region: not a region operation");
        }
        size_t elem = snapshotTypedElemSize(r.dataType);
        if (elem == 0) {
            throw FaabricException(
              "device merge region: typed operation needs Int, Long, "
              "Float or Double");
        }
        if ((r.offset % elem) != 0) {
            throw FaabricException("device merge region: unaligned offset");
        }
        if ((size_t)r.offset >= arenaSize) {
            throw FaabricException(
              "device merge region: offset outside the arena");
        }
        typed.push_back(r);
    }
    std::sort(typed.begin(),
              typed.end(),
              [](const SnapshotMergeRegion& a, const SnapshotMergeRegion& b) {
                  return a.offset < b.offset;
              });
    auto endOf = [arenaSize](const SnapshotMergeRegion& r) {
        return r.length == 0
                 ? arenaSize
                 : std::min(arenaSize, (size_t)r.offset + r.length);
    };
    for (size_t i = 1; i < typed.size(); i++) {
        if (endOf(typed[i - 1]) > (size_t)typed[i].offset) {
            throw FaabricException(
              "device merge region: typed regions overlap");
        }
    }
    return typed;
}

void DeviceSnapshot::ensureTypedScratch(size_t count, size_t elemSize)
{
    if (typedCtl_ == nullptr) {
        OPS_HIP_CHECK(hipMalloc(&typedCtl_, 2 * sizeof(uint32_t)));
    }
    if (count > typedIdxCap_) {
        if (typedIdx_ != nullptr) {
            hipFree(typedIdx_);
            typedIdx_ = nullptr;
            typedIdxCap_ = 0;
        }
        OPS_HIP_CHECK(hipMalloc(&typedIdx_, count * sizeof(uint32_t)));
        typedIdxCap_ = count;
    }
    if (count * elemSize > typedValCap_) {
        if (typedVal_ != nullptr) {
            hipFree(typedVal_);
            typedVal_ = nullptr;
            typedValCap_ = 0;
        }
        OPS_HIP_CHECK(hipMalloc(&typedVal_, count * elemSize));
        typedValCap_ = count * elemSize;
    }
}

std::optional<SnapshotDiff> DeviceSnapshot::typedDiff(
  const void* devPtr,
  const SnapshotMergeRegion& region)
{
    size_t elem = snapshotTypedElemSize(region.dataType);
    if (elem == 0 || !isTypedMergeOperation(region.operation)) {
        throw FaabricException("typed diff: not a typed merge region");
    }
    if ((region.offset % elem) != 0) {
        throw FaabricException("typed diff: unaligned region offset");
    }
    if ((size_t)region.offset >= bytes_) {
        throw FaabricException("typed diff: region outside the snapshot");
    }
    size_t end = region.length == 0
                   ? bytes_
                   : std::min(bytes_, (size_t)region.offset + region.length);
    // Trailing bytes that do not fill an element are diffed by nothing
    size_t nElems = (end - region.offset) / elem;
    if (nElems == 0) {
        return std::nullopt;
    }
    if (nElems > 0xffffffffull) {
        throw FaabricException("typed diff: region too large");
    }

    std::lock_guard<std::recursive_mutex> lock(typedMx_);
    OPS_HIP_CHECK(hipSetDevice(device_));
    ensureTypedScratch(nElems, elem);
    OPS_HIP_CHECK(
      hipMemsetAsync(typedCtl_, 0, 2 * sizeof(uint32_t), stream_));
    OPS_HIP_CHECK(famTypedDiff(snap_,
                               devPtr,
                               region.offset,
                               nElems,
                               (int)region.dataType,
                               (int)region.operation,
                               typedCtl_,
                               typedCtl_ + 1,
                               typedIdx_,
                               typedVal_,
                               stream_));
    uint32_t ctl[2] = { 0, 0 };
    OPS_HIP_CHECK(hipMemcpyAsync(
      ctl, typedCtl_, sizeof(ctl), hipMemcpyDeviceToHost, stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
    if (ctl[1] != 0) {
        throw FaabricException("product diff with zero original");
    }
    uint32_t count = ctl[0];
    if (count == 0) {
        return std::nullopt;
    }
    if (count > nElems) {
        throw FaabricException("typed diff: entry count past the region");
    }

    SnapshotDiff diff;
    diff.dataType = region.dataType;
    diff.operation = SnapshotMergeOperation::TypedElems;
    diff.offset = region.offset;
    diff.dataCopy.assign(typedElemsPackedSize(count, elem), 0);
    uint32_t op = (uint32_t)region.operation;
    std::memcpy(diff.dataCopy.data(), &op, 4);
    std::memcpy(diff.dataCopy.data() + 4, &count, 4);
    OPS_HIP_CHECK(hipMemcpyAsync(diff.dataCopy.data() + 8,
                                 typedIdx_,
                                 (size_t)count * 4,
                                 hipMemcpyDeviceToHost,
                                 stream_));
    OPS_HIP_CHECK(hipMemcpyAsync(
      diff.dataCopy.data() + diff.dataCopy.size() - (size_t)count * elem,
      typedVal_,
      (size_t)count * elem,
      hipMemcpyDeviceToHost,
      stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
    return diff;
}

void DeviceSnapshot::applyTypedDiff(const SnapshotDiff& diff)
{
    if (diff.operation != SnapshotMergeOperation::TypedElems) {
        throw FaabricException("not a typed elems diff");
    }
    // Nothing is uploaded or applied before the whole diff is checked
    TypedElemsView v = validateTypedElemsDiff(diff, bytes_);
    if (v.count == 0) {
        return;
    }
    std::lock_guard<std::recursive_mutex> lock(typedMx_);
    OPS_HIP_CHECK(hipSetDevice(device_));
    ensureTypedScratch(v.count, v.elemSize);
    OPS_HIP_CHECK(hipMemcpyAsync(typedIdx_,
                                 v.idx,
                                 (size_t)v.count * 4,
                                 hipMemcpyHostToDevice,
                                 stream_));
    OPS_HIP_CHECK(hipMemcpyAsync(typedVal_,
                                 v.values,
                                 (size_t)v.count * v.elemSize,
                                 hipMemcpyHostToDevice,
                                 stream_));
    OPS_HIP_CHECK(famApplyTypedElems(snap_ + diff.offset,
                                     typedIdx_,
                                     typedVal_,
                                     v.count,
                                     (int)diff.dataType,
                                     (int)v.op,
                                     stream_));
    OPS_HIP_CHECK(hipStreamSynchronize(stream_));
}

std::vector<SnapshotDiff> DeviceSnapshot::diffWithRegions(
  const void* devPtr,
  const std::vector<SnapshotMergeRegion>& regions)
{
    std::vector<SnapshotMergeRegion> typed =
      validateDeviceMergeRegions(regions, bytes_);
    std::lock_guard<std::recursive_mutex> lock(typedMx_);

    std::vector<SnapshotDiff> diffs;
    for (const auto& r : typed) {
        auto d = typedDiff(devPtr, r);
        if (d.has_value()) {
            diffs.push_back(std::move(*d));
        }
    }

    // Everything else ships as XOR pages, with the typed bytes taken out:
    // their change already travels as a typed diff
    uint32_t nd = diffXor(devPtr);
    if (nd == 0) {
        return diffs;
    }
    if (!typed.empty()) {
        // Typed byte ranges [begin, end), sorted; touching ones merged so
        // a page covered by two adjacent regions counts as wholly typed
        std::vector<std::pair<size_t, size_t>> ranges;
        for (const auto& r : typed) {
            size_t end = r.length == 0
                           ? bytes_
                           : std::min(bytes_, (size_t)r.offset + r.length);
            // The sparse payload is indexed by page, so arena offsets
            // apply directly
            OPS_HIP_CHECK(hipMemsetAsync(
              payload_ + r.offset, 0, end - r.offset, stream_));
            if (!ranges.empty() && ranges.back().second == r.offset) {
                ranges.back().second = end;
            } else {
                ranges.emplace_back(r.offset, end);
            }
        }
        std::vector<uint32_t> pages(nd);
        OPS_HIP_CHECK(hipMemcpyAsync(pages.data(),
                                     pageIdx_,
                                     (size_t)nd * 4,
                                     hipMemcpyDeviceToHost,
                                     stream_));
        OPS_HIP_CHECK(hipStreamSynchronize(stream_));
        std::vector<uint32_t> kept;
        kept.reserve(nd);
        for (uint32_t p : pages) {
            size_t pLo = (size_t)p * DEVICE_PAGE;
            size_t pHi = pLo + DEVICE_PAGE;
            bool whollyTyped = false;
            for (const auto& [lo, hi] : ranges) {
                if (lo <= pLo && pHi <= hi) {
                    whollyTyped = true;
                    break;
                }
            }
            if (!whollyTyped) {
                kept.push_back(p);
            }
        }
        if (!kept.empty()) {
            OPS_HIP_CHECK(hipMemcpyAsync(pageIdx_,
                                         kept.data(),
                                         kept.size() * 4,
                                         hipMemcpyHostToDevice,
                                         stream_));
            OPS_HIP_CHECK(hipStreamSynchronize(stream_));
        }
        lastDirty_ = (uint32_t)kept.size();
        if (kept.empty()) {
            return diffs;
        }
    }

    std::vector<uint32_t> pages;
    std::vector<uint8_t> payload;
    gatherLastDiffToHost(pages, payload);
    uint32_t n = (uint32_t)pages.size();
    SnapshotDiff xd;
    xd.dataType = SnapshotDataType::Raw;
    xd.operation = SnapshotMergeOperation::XorPages;
    xd.offset = 0;
    xd.dataCopy.resize(4 + (size_t)n * 4 + payload.size());
    std::memcpy(xd.dataCopy.data(), &n, 4);
    std::memcpy(xd.dataCopy.data() + 4, pages.data(), (size_t)n * 4);
    std::memcpy(
      xd.dataCopy.data() + 4 + (size_t)n * 4, payload.data(), payload.size());
    diffs.push_back(std::move(xd));
    return diffs;
}

void DeviceSnapshot::queueDiff(SnapshotDiff diff)
{
    if (diff.operation != SnapshotMergeOperation::XorPages &&
        diff.operation != SnapshotMergeOperation::TypedElems) {
        throw FaabricException(
          "device snapshots queue XorPages and TypedElems diffs only");
    }
    std::lock_guard<std::mutex> lock(queueMx_);
    queued_.push_back(std::move(diff));
}

void DeviceSnapshot::queuePackedDiff(std::vector<uint8_t> packed)
{
    SnapshotDiff d;
    d.dataType = SnapshotDataType::Raw;
    d.operation = SnapshotMergeOperation::XorPages;
    d.dataCopy = std::move(packed);
    queueDiff(std::move(d));
}

int DeviceSnapshot::applyQueuedPackedDiffs()
{
    std::vector<SnapshotDiff> toApply;
    {
        std::lock_guard<std::mutex> lock(queueMx_);
        toApply.swap(queued_);
    }
    for (const auto& diff : toApply) {
        if (diff.operation == SnapshotMergeOperation::TypedElems) {
            applyTypedDiff(diff);
            continue;
        }
        const std::vector<uint8_t>& packed = diff.dataCopy;
        if (packed.size() < 4) {
            continue;
        }
        uint32_t n = 0;
        std::memcpy(&n, packed.data(), 4);
        size_t headerBytes = 4 + (size_t)n * 4;
        if (packed.size() < headerBytes + (size_t)n * DEVICE_PAGE) {
            throw FaabricException("bad packed diff");
        }
        std::vector<uint32_t> pages(n);
        std::memcpy(pages.data(), packed.data() + 4, (size_t)n * 4);
        applyCompactDiffFromHost(pages,
                                 packed.data() + headerBytes,
                                 (size_t)n * DEVICE_PAGE);
    }
    return (int)toApply.size();
}

DeviceSnapshotRegistry& DeviceSnapshotRegistry::get()
{
    static DeviceSnapshotRegistry reg;
    return reg;
}

std::shared_ptr<DeviceSnapshot> DeviceSnapshotRegistry::getSnapshot(
  const std::string& key)
{
    std::lock_guard<std::mutex> lock(mx);
    auto it = snapshots.find(key);
    if (it == snapshots.end()) {
        throw FaabricException("device snapshot not found: " + key);
    }
    return it->second;
}

bool DeviceSnapshotRegistry::snapshotExists(const std::string& key)
{
    std::lock_guard<std::mutex> lock(mx);
    return snapshots.count(key) > 0;
}

void DeviceSnapshotRegistry::registerSnapshot(
  const std::string& key,
  std::shared_ptr<DeviceSnapshot> snap)
{
    std::lock_guard<std::mutex> lock(mx);
    snapshots[key] = std::move(snap);
}

void DeviceSnapshotRegistry::deleteSnapshot(const std::string& key)
{
    std::lock_guard<std::mutex> lock(mx);
    snapshots.erase(key);
    mergeRegions.erase(key);
}

void DeviceSnapshotRegistry::clear()
{
    std::lock_guard<std::mutex> lock(mx);
    snapshots.clear();
    mergeRegions.clear();
}

void DeviceSnapshotRegistry::setMergeRegions(
  const std::string& key,
  const std::vector<SnapshotMergeRegion>& regions)
{
    std::lock_guard<std::mutex> lock(mx);
    if (regions.empty()) {
        mergeRegions.erase(key);
    } else {
        mergeRegions[key] = regions;
    }
}

std::vector<SnapshotMergeRegion> DeviceSnapshotRegistry::getMergeRegions(
  const std::string& key)
{
    std::lock_guard<std::mutex> lock(mx);
    auto it = mergeRegions.find(key);
    if (it == mergeRegions.end()) {
        return {};
    }
    return it->second;
}

void deviceElementwiseOp(void* inout,
                         const void* in,
                         uint64_t count,
                         int dtype,
                         int op,
                         hipStream_t stream)
{
    OPS_HIP_CHECK(famElementwiseOp(inout, in, count, dtype, op, stream));
    OPS_HIP_CHECK(hipStreamSynchronize(stream));
}

} // namespace faabricamd

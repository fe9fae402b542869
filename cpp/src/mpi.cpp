// MPI world implementation (reference behavior: src/mpi/MpiWorld.cpp —
// create :157-226, init :270-300, send/recv :544-705, collectives
// :786-1484, op_reduce :1266-1389, barrier :1753-1775;
// src/mpi/MpiWorldRegistry.cpp; src/mpi/MpiContext.cpp). See mpi.h for
// the MI355X re-design notes (host plane on the PTP broker, device plane
// on RCCL over xGMI).
#include "faabricamd/mpi.h"
#include "faabricamd/utilextras.h"
#include "faabricamd/ops.h"
#include "faabricamd/executor.h"
#include "faabricamd/planner.h"
#include "faabricamd/ptp.h"
#include "faabricamd/util.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>

namespace faabricamd {

size_t mpiTypeSize(MpiDataType t)
{
    switch (t) {
        case MpiDataType::INT32:
            return 4;
        case MpiDataType::INT64:
        case MpiDataType::UINT64:
        case MpiDataType::DOUBLE:
            return 8;
        case MpiDataType::FLOAT:
            return 4;
        case MpiDataType::BYTE:
            return 1;
    }
    return 1;
}

static ncclDataType_t toNccl(MpiDataType t)
{
    switch (t) {
        case MpiDataType::INT32:
            return ncclInt32;
        case MpiDataType::INT64:
            return ncclInt64;
        case MpiDataType::UINT64:
            return ncclUint64;
        case MpiDataType::FLOAT:
            return ncclFloat32;
        case MpiDataType::DOUBLE:
            return ncclFloat64;
        case MpiDataType::BYTE:
            return ncclUint8;
    }
    return ncclUint8;
}

static ncclRedOp_t toNcclOp(MpiOp op)
{
    switch (op) {
        case MpiOp::SUM:
            return ncclSum;
        case MpiOp::MAX:
            return ncclMax;
        case MpiOp::MIN:
            return ncclMin;
        case MpiOp::PROD:
            return ncclProd;
    }
    return ncclSum;
}

#define RCCL_CHECK(call)                                                       \
    do {                                                                       \
        ncclResult_t rcclRes_ = (call);                                        \
        if (rcclRes_ != ncclSuccess) {                                         \
            throw FaabricException(std::string("RCCL error: ") +               \
                                   ncclGetErrorString(rcclRes_));              \
        }                                                                      \
    } while (0)

#define HIP_CHECK(call)                                                        \
    do {                                                                       \
        hipError_t hipRes_ = (call);                                           \
        if (hipRes_ != hipSuccess) {                                           \
            throw FaabricException(std::string("HIP error: ") +                \
                                   hipGetErrorString(hipRes_));                \
        }                                                                      \
    } while (0)

// Host-plane channel namespace: sendIdx = sendRank + type * MAX_WORLD_SIZE
static int32_t chanSendIdx(int sendRank, MpiMessageType type)
{
    return sendRank + (int32_t)type * MAX_MPI_WORLD_SIZE;
}

// ------------------------- per-rank TLS state -------------------------------

struct PendingRecv
{
    int requestId = 0;
    int sendRank = 0;
    int recvRank = 0;
    uint8_t* buffer = nullptr;
    size_t bytes = 0;
    MpiMessageType type = MpiMessageType::NORMAL;
    bool done = false;
    bool onDevice = false; // drain via the device plane (devRecv)
};

// Async request bookkeeping per rank-thread
// (reference: MpiRankState src/mpi/MpiWorld.cpp:45-113)
struct MpiRankState
{
    std::vector<PendingRecv> pendingRecvs;
    // Stream-ordered RCCL requests: requestId → hipEvent_t recorded
    // after the enqueued ncclSend/Recv (awaited, then destroyed)
    std::map<int, hipEvent_t> deviceEvents;
    std::atomic<int> nextRequestId{ 1 };
};

static thread_local MpiRankState rankState;

// ------------------------- RCCL state ---------------------------------------

struct MpiWorld::RcclState
{
    std::mutex mx;
    ncclUniqueId uniqueId;
    std::map<int, ncclComm_t> comms;      // world rank → comm
    std::map<int, hipStream_t> streams;   // world rank → stream
    std::map<int, int> devices;           // world rank → hip device
    ~RcclState()
    {
        for (auto& [rank, comm] : comms) {
            ncclCommDestroy(comm);
        }
        for (auto& [rank, stream] : streams) {
            hipStreamDestroy(stream);
        }
    }
};

// ------------------------- world lifecycle ----------------------------------

MpiWorld::MpiWorld()
  : thisHost(getSystemConfig().endpointHost)
{}

MpiWorld::~MpiWorld() = default;

void MpiWorld::create(Message& call, int newId, int newSize)
{
    if (newSize > MAX_MPI_WORLD_SIZE) {
        throw FaabricException("MPI world size exceeds cap");
    }
    id = newId;
    size = newSize;
    appId = call.appId;
    user = call.user;
    function = call.function;

    call.isMpi = true;
    call.mpiWorldId = id;
    call.mpiRank = 0;
    call.mpiWorldSize = size;

    // Dispatch the other ranks: SCALE_CHANGE consuming the planner's
    // preloaded gang decision (reference: src/mpi/MpiWorld.cpp:157-226)
    auto req = std::make_shared<BatchExecuteRequest>();
    req->appId = appId;
    req->user = user;
    req->function = function;
    req->type = BatchExecuteType::FUNCTIONS;
    for (int i = 1; i < size; i++) {
        Message m = messageFactory(user, function);
        m.appId = appId;
        m.appIdx = i;
        m.groupIdx = i;
        m.isMpi = true;
        m.mpiWorldId = id;
        m.mpiRank = i;
        m.mpiWorldSize = size;
        m.inputData = call.inputData;
        m.recordExecGraph = call.recordExecGraph;
        req->messages.push_back(std::move(m));
    }

    auto decision = getPlannerClient().callFunctions(req);
    if (decision->appId == NOT_ENOUGH_SLOTS) {
        throw FaabricException("not enough slots to create MPI world");
    }
    groupId = decision->groupId;
    call.groupId = groupId;
    call.groupSize = size;

    getPointToPointBroker().waitForMappingsOnThisHost(groupId);
    {
        std::lock_guard<std::mutex> lock(worldMx);
        localRanks.push_back(0);
    }
}

void MpiWorld::initialiseFromMsg(Message& msg)
{
    id = msg.mpiWorldId;
    size = msg.mpiWorldSize;
    appId = msg.appId;
    groupId = msg.groupId;
    user = msg.user;
    function = msg.function;
    getPointToPointBroker().waitForMappingsOnThisHost(groupId);
}

void MpiWorld::initialiseRankFromMsg(Message& msg)
{
    {
        std::lock_guard<std::mutex> lock(worldMx);
        if (std::find(localRanks.begin(), localRanks.end(), msg.mpiRank) ==
            localRanks.end()) {
            localRanks.push_back(msg.mpiRank);
        }
    }
    // Spin-poll mode burns the rank's core on purpose; pin it so the
    // spinner and the scheduler don't migrate each other around
    // (reference: src/mpi/MpiWorld.cpp:292-296 pins under
    // FAABRIC_USE_SPINLOCK)
    static const bool useSpin =
      getEnvVarInt("FAABRIC_USE_SPINLOCK", 0) != 0;
    if (useSpin) {
        pinThreadToFreeCpu();
    }
}

// host → ranks on that host (rank-ascending). The first rank on each
// host is its local leader (reference: initLocalRemoteLeaders,
// src/mpi/MpiWorld.cpp:318-367). Every process derives the same map
// from the group mappings, so leaders and batch layouts agree.
std::map<std::string, std::vector<int>> MpiWorld::ranksPerHost()
{
    std::map<std::string, std::vector<int>> out;
    for (int r = 0; r < size; r++) {
        out[getHostForRank(r)].push_back(r);
    }
    return out;
}

std::string MpiWorld::getHostForRank(int rank)
{
    {
        std::lock_guard<std::mutex> lock(worldMx);
        if ((int)rankHosts.size() == size && !rankHosts[rank].empty()) {
            return rankHosts[rank];
        }
    }
    std::string host = getPointToPointBroker().getHostForReceiver(groupId,
                                                                  rank);
    std::lock_guard<std::mutex> lock(worldMx);
    if ((int)rankHosts.size() != size) {
        rankHosts.assign(size, "");
    }
    rankHosts[rank] = host;
    return host;
}

bool MpiWorld::destroy()
{
    std::lock_guard<std::mutex> lock(worldMx);
    localRanks.clear();
    rccl.reset();
    if (fbStream_ != nullptr) {
        (void)hipStreamDestroy((hipStream_t)fbStream_);
        fbStream_ = nullptr;
    }
    return true;
}

bool MpiWorld::rankFinished(int rank)
{
    // Called by the executor when a rank's function completes; once the
    // last LOCAL rank is done this host's world state (incl. RCCL comms
    // and streams) is released and the caller clears the registry entry
    // (reference: executor-side MPI cleanup)
    std::lock_guard<std::mutex> lock(worldMx);
    auto it = std::find(localRanks.begin(), localRanks.end(), rank);
    if (it != localRanks.end()) {
        localRanks.erase(it);
    }
    if (!localRanks.empty()) {
        return false;
    }
    rccl.reset();
    if (fbStream_ != nullptr) {
        (void)hipStreamDestroy((hipStream_t)fbStream_);
        fbStream_ = nullptr;
    }
    return true;
}

// ------------------------- cartesian topology -------------------------------

void MpiWorld::setCartesianDims(int ndims, const int* dims)
{
    // Validate the grid covers the world exactly, then store it. The
    // reference stores dims on first use and requires dims[0]*dims[1] ==
    // size (src/mpi/MpiWorld.cpp:379-395); we accept any N-dim row-major
    // grid with the same product rule.
    long product = 1;
    for (int d = 0; d < ndims; d++) {
        if (dims[d] <= 0) {
            throw FaabricException("cartesian dim must be positive");
        }
        product *= dims[d];
    }
    if (product != size) {
        throw FaabricException(
          "product of cartesian dims does not equal world size");
    }
    std::lock_guard<std::mutex> lock(cartMx);
    cartDims.assign(dims, dims + ndims);
}

// Stored dims, defaulting to a 1-D {size} layout before any Cart call
static std::vector<int> effectiveDims(std::mutex& mx,
                                      const std::vector<int>& stored,
                                      int size)
{
    std::lock_guard<std::mutex> lock(mx);
    if (stored.empty()) {
        return { size };
    }
    return stored;
}

void MpiWorld::getCartesianRank(int rank,
                                int maxDims,
                                const int* dims,
                                int* periods,
                                int* coords)
{
    // Row-major cartesian layout (reference: src/mpi/MpiWorld.cpp:369-450)
    if (rank >= size) {
        throw FaabricException("rank out of world");
    }
    setCartesianDims(maxDims, dims);
    int remainder = rank;
    for (int d = 0; d < maxDims; d++) {
        int stride = 1;
        for (int e = d + 1; e < maxDims; e++) {
            stride *= dims[e];
        }
        coords[d] = remainder / stride;
        remainder = remainder % stride;
        periods[d] = 1; // always periodic, like the reference (LAMMPS)
    }
}

void MpiWorld::getCartesianGrid(int rank,
                                int maxDims,
                                int* dims,
                                int* periods,
                                int* coords)
{
    std::vector<int> eff = effectiveDims(cartMx, cartDims, size);
    int remainder = rank;
    for (int d = 0; d < maxDims; d++) {
        int dim = d < (int)eff.size() ? eff[d] : 1;
        dims[d] = dim;
        int stride = 1;
        for (int e = d + 1; e < (int)eff.size(); e++) {
            stride *= eff[e];
        }
        if (d < (int)eff.size()) {
            coords[d] = remainder / stride;
            remainder = remainder % stride;
        } else {
            coords[d] = 0;
        }
        periods[d] = 1;
    }
}

void MpiWorld::getRankFromCoords(int* rank, int* coords)
{
    // Row-major fold using the stored dims (inverse of getCartesianRank).
    // Reference: *rank = coords[1] + coords[0]*dims[1] for its 2-D grids
    // (src/mpi/MpiWorld.cpp:422-438); this is the N-dim generalisation.
    std::vector<int> eff = effectiveDims(cartMx, cartDims, size);
    int r = 0;
    for (size_t d = 0; d < eff.size(); d++) {
        r = r * eff[d] + coords[d];
    }
    *rank = r;
}

void MpiWorld::shiftCartesianCoords(int rank,
                                    int direction,
                                    int disp,
                                    int* source,
                                    int* destination)
{
    // source = the rank that reaches me moving disp units in direction;
    // destination = the rank I reach. Periodic in every dimension
    // (reference: src/mpi/MpiWorld.cpp:440-490).
    std::vector<int> eff = effectiveDims(cartMx, cartDims, size);
    int ndims = (int)eff.size();

    // Decompose my rank into row-major coords
    std::vector<int> coords(ndims);
    int remainder = rank;
    for (int d = 0; d < ndims; d++) {
        int stride = 1;
        for (int e = d + 1; e < ndims; e++) {
            stride *= eff[e];
        }
        coords[d] = remainder / stride;
        remainder = remainder % stride;
    }

    auto fold = [&](const std::vector<int>& c) {
        int r = 0;
        for (int d = 0; d < ndims; d++) {
            r = r * eff[d] + c[d];
        }
        return r;
    };

    if (direction < 0 || direction >= ndims) {
        // Unused dimension: single process there, periodicity lands on self
        *source = rank;
        *destination = rank;
        return;
    }

    int dim = eff[direction];
    // Normalise disp into [0, dim) so negative displacements wrap
    int step = ((disp % dim) + dim) % dim;

    std::vector<int> fwd = coords;
    fwd[direction] = (coords[direction] + step) % dim;
    *destination = fold(fwd);

    std::vector<int> bwd = coords;
    bwd[direction] = (coords[direction] - step + dim) % dim;
    *source = fold(bwd);
}

// ------------------------- host data plane ----------------------------------

void MpiWorld::hostSend(int sendRank,
                        int recvRank,
                        const uint8_t* buffer,
                        size_t bytes,
                        MpiMessageType messageType)
{
    getPointToPointBroker().sendMessage(appId,
                                        groupId,
                                        chanSendIdx(sendRank, messageType),
                                        recvRank,
                                        buffer,
                                        bytes,
                                        /*mustOrderMsgs=*/true);
}

std::vector<uint8_t> MpiWorld::hostRecv(int sendRank,
                                        int recvRank,
                                        size_t expectedBytes,
                                        MpiMessageType messageType)
{
    auto data = getPointToPointBroker().recvMessage(
      groupId,
      chanSendIdx(sendRank, messageType),
      recvRank,
      /*mustOrderMsgs=*/true,
      getSystemConfig().globalMessageTimeout);
    if (expectedBytes > 0 && data.size() > expectedBytes) {
        throw FaabricException("mpi recv buffer too small");
    }
    return data;
}

// ------------------------- device plane (RCCL) ------------------------------

bool MpiWorld::isDeviceBuffer(const void* ptr, MpiBufferLoc loc)
{
    if (loc == MpiBufferLoc::HOST) {
        return false;
    }
    if (loc == MpiBufferLoc::DEVICE) {
        return true;
    }
    hipPointerAttribute_t attrs;
    if (hipPointerGetAttributes(&attrs, ptr) != hipSuccess) {
        (void)hipGetLastError(); // clear
        return false;
    }
    return attrs.type == hipMemoryTypeDevice;
}

void MpiWorld::ensureRcclComm(int rank)
{
    {
        std::lock_guard<std::mutex> lock(worldMx);
        if (!rccl) {
            rccl = std::make_shared<RcclState>();
        }
    }
    {
        std::lock_guard<std::mutex> lock(rccl->mx);
        if (rccl->comms.count(rank) > 0) {
            return;
        }
    }

    // Device for this rank: each worker process owns its GPU(s); ranks
    // local to a process spread over visible devices in local-rank order
    int nDevices = 0;
    HIP_CHECK(hipGetDeviceCount(&nDevices));
    if (nDevices == 0) {
        throw FaabricException("RCCL path requires a GPU");
    }
    int device;
    {
        std::lock_guard<std::mutex> lock(worldMx);
        auto it = std::find(localRanks.begin(), localRanks.end(), rank);
        int localIdx =
          it == localRanks.end()
            ? 0
            : (int)std::distance(localRanks.begin(), it);
        // Base device from config (all-visible deployments set
        // FAABRIC_GPU_DEVICE per worker); extra local ranks spread
        device = (getSystemConfig().gpuDevice + localIdx) % nDevices;
    }
    HIP_CHECK(hipSetDevice(device));

    // Bootstrap: rank 0 generates the uniqueId and ships it to every
    // other rank over the host plane (replaces the reference's full-mesh
    // TCP handshake, src/mpi/MpiWorld.cpp:1789-1935)
    ncclUniqueId uid;
    if (rank == 0) {
        RCCL_CHECK(ncclGetUniqueId(&uid));
        for (int i = 1; i < size; i++) {
            hostSend(0,
                     i,
                     (const uint8_t*)&uid,
                     sizeof(uid),
                     MpiMessageType::HANDSHAKE);
        }
    } else {
        auto data = hostRecv(0, rank, sizeof(uid),
                             MpiMessageType::HANDSHAKE);
        std::memcpy(&uid, data.data(), sizeof(uid));
    }

    ncclComm_t comm;
    RCCL_CHECK(ncclCommInitRank(&comm, size, uid, rank));
    hipStream_t stream;
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));

    std::lock_guard<std::mutex> lock(rccl->mx);
    rccl->comms[rank] = comm;
    rccl->streams[rank] = stream;
    rccl->devices[rank] = device;
}

bool MpiWorld::rcclUsable(int rank)
{
    static const int forced = []() {
        const char* e = getenv("FAABRIC_DEVICE_PLANE");
        if (e == nullptr) {
            return 0; // auto
        }
        if (strcmp(e, "rccl") == 0) {
            return 1;
        }
        if (strcmp(e, "ptp") == 0) {
            return -1;
        }
        return 0;
    }();
    if (forced == -1) {
        return false;
    }
    {
        std::lock_guard<std::mutex> lock(worldMx);
        if (rcclBroken) {
            return false;
        }
    }
    if (forced == 1) {
        ensureRcclComm(rank); // throw loudly if forced and unavailable
        return true;
    }
    try {
        ensureRcclComm(rank);
        return true;
    } catch (const std::exception& e) {
        // Typical cause: ranks sharing one GPU — RCCL refuses duplicate
        // devices. The PTP/IPC device plane takes over for this world.
        FAM_WARN("world %d: RCCL unavailable for rank %d (%s); using the "
                 "PTP/IPC device plane",
                 id,
                 rank,
                 e.what());
        std::lock_guard<std::mutex> lock(worldMx);
        rcclBroken = true;
        return false;
    }
}

void* MpiWorld::fallbackStream()
{
    std::lock_guard<std::mutex> lock(worldMx);
    if (fbStream_ == nullptr) {
        hipStream_t s = nullptr;
        HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        fbStream_ = (void*)s;
    }
    return fbStream_;
}

void MpiWorld::devSend(int sendRank,
                       int recvRank,
                       const void* devPtr,
                       size_t bytes,
                       MpiMessageType type)
{
    getPointToPointBroker().sendMessageDevice(appId,
                                              groupId,
                                              chanSendIdx(sendRank, type),
                                              recvRank,
                                              devPtr,
                                              bytes,
                                              /*mustOrderMsgs=*/true);
}

void MpiWorld::devRecv(int sendRank,
                       int recvRank,
                       void* devPtr,
                       size_t bytes,
                       MpiMessageType type)
{
    size_t got = getPointToPointBroker().recvMessageDevice(
      groupId,
      chanSendIdx(sendRank, type),
      recvRank,
      devPtr,
      bytes,
      /*mustOrderMsgs=*/true,
      getSystemConfig().globalMessageTimeout);
    if (got != bytes) {
        throw FaabricException("device-plane recv size mismatch");
    }
}

void MpiWorld::deviceReduceFallback(int thisRank,
                                    int rootRank,
                                    const uint8_t* sendBuffer,
                                    uint8_t* recvBuffer,
                                    MpiDataType dataType,
                                    int count,
                                    MpiOp op)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    if (bytes == 0) {
        return; // the count is the same on every rank: nothing to fold
    }
    if (thisRank != rootRank) {
        devSend(thisRank, rootRank, sendBuffer, bytes,
                MpiMessageType::REDUCE);
        return;
    }
    hipStream_t s = (hipStream_t)fallbackStream();
    if (recvBuffer != sendBuffer) {
        HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    uint8_t* scratch = nullptr;
    HIP_CHECK(hipMallocAsync((void**)&scratch, bytes, s));
    for (int i = 0; i < size; i++) {
        if (i == rootRank) {
            continue;
        }
        devRecv(i, rootRank, scratch, bytes, MpiMessageType::REDUCE);
        // Fused on-GPU combine (gfx950 elementwise kernel); syncs
        deviceElementwiseOp(recvBuffer, scratch, (uint64_t)count,
                            (int)dataType, (int)op, s);
    }
    HIP_CHECK(hipFreeAsync(scratch, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

void MpiWorld::deviceBroadcastFallback(int rootRank,
                                       int thisRank,
                                       uint8_t* buffer,
                                       size_t bytes,
                                       MpiMessageType type)
{
    if (thisRank == rootRank) {
        for (int i = 0; i < size; i++) {
            if (i != rootRank) {
                devSend(rootRank, i, buffer, bytes, type);
            }
        }
    } else {
        devRecv(rootRank, thisRank, buffer, bytes, type);
    }
}

void* MpiWorld::getRcclComm(int rank)
{
    ensureRcclComm(rank);
    std::lock_guard<std::mutex> lock(rccl->mx);
    return (void*)rccl->comms.at(rank);
}

void* MpiWorld::getRankStream(int rank)
{
    ensureRcclComm(rank);
    std::lock_guard<std::mutex> lock(rccl->mx);
    return (void*)rccl->streams.at(rank);
}

// ------------------------- point-to-point -----------------------------------

void MpiWorld::send(int sendRank,
                    int recvRank,
                    const uint8_t* buffer,
                    MpiDataType dataType,
                    int count,
                    MpiMessageType messageType,
                    MpiBufferLoc loc)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    recordMsgCount(sendRank, recvRank, messageType);
    if (isDeviceBuffer(buffer, loc)) {
        if (!rcclUsable(sendRank)) {
            devSend(sendRank, recvRank, buffer, bytes, messageType);
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(sendRank);
            stream = rccl->streams.at(sendRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(sendRank)));
        }
        RCCL_CHECK(ncclSend(
          buffer, count, toNccl(dataType), recvRank, comm, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    hostSend(sendRank, recvRank, buffer, bytes, messageType);
}

void MpiWorld::recv(int sendRank,
                    int recvRank,
                    uint8_t* buffer,
                    MpiDataType dataType,
                    int count,
                    MpiMessageType messageType,
                    MpiBufferLoc loc)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    bool onDevice = isDeviceBuffer(buffer, loc);
    if (onDevice && rcclUsable(recvRank)) {
        // The rank stream orders this receive after any earlier irecv
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(recvRank);
            stream = rccl->streams.at(recvRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(recvRank)));
        }
        RCCL_CHECK(ncclRecv(
          buffer, count, toNccl(dataType), sendRank, comm, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }

    // Pending irecvs on this channel must drain first to preserve MPI
    // matching order, on the host plane and the PTP device plane alike
    // (reference: recvBatchReturnLast src/mpi/MpiWorld.cpp:1963-2030)
    for (auto& p : rankState.pendingRecvs) {
        if (!p.done && p.sendRank == sendRank && p.recvRank == recvRank &&
            p.type == messageType) {
            if (p.onDevice) {
                devRecv(sendRank, recvRank, p.buffer, p.bytes,
                        messageType);
            } else {
                auto data =
                  hostRecv(sendRank, recvRank, p.bytes, messageType);
                std::memcpy(p.buffer, data.data(), data.size());
            }
            p.done = true;
        }
    }
    if (onDevice) {
        devRecv(sendRank, recvRank, buffer, bytes, messageType);
        return;
    }
    auto data = hostRecv(sendRank, recvRank, bytes, messageType);
    std::memcpy(buffer, data.data(), data.size());
}

int MpiWorld::isend(int sendRank,
                    int recvRank,
                    const uint8_t* buffer,
                    MpiDataType dataType,
                    int count,
                    MpiMessageType messageType,
                    MpiBufferLoc loc)
{
    int id = rankState.nextRequestId.fetch_add(1);
    if (isDeviceBuffer(buffer, loc)) {
        if (rcclUsable(sendRank)) {
            // True async: enqueue on the rank stream, record an event,
            // return. No sync inside isend (reference semantics:
            // per-rank unacked buffers, src/mpi/MpiWorld.cpp:45-113)
            ncclComm_t comm;
            hipStream_t stream;
            {
                std::lock_guard<std::mutex> lock(rccl->mx);
                comm = rccl->comms.at(sendRank);
                stream = rccl->streams.at(sendRank);
                HIP_CHECK(hipSetDevice(rccl->devices.at(sendRank)));
            }
            RCCL_CHECK(ncclSend(buffer, count, toNccl(dataType),
                                recvRank, comm, stream));
            hipEvent_t ev;
            HIP_CHECK(
              hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(ev, stream));
            rankState.deviceEvents[id] = ev;
            return id;
        }
        // Fallback plane sends are buffered (staged copy + control
        // message; the sender's buffer is immediately reusable)
        devSend(sendRank, recvRank, buffer,
                mpiTypeSize(dataType) * (size_t)count, messageType);
        return id;
    }
    // Buffered eager send: completes immediately
    send(sendRank, recvRank, buffer, dataType, count, messageType);
    return id;
}

int MpiWorld::irecv(int sendRank,
                    int recvRank,
                    uint8_t* buffer,
                    MpiDataType dataType,
                    int count,
                    MpiMessageType messageType,
                    MpiBufferLoc loc)
{
    PendingRecv p;
    p.requestId = rankState.nextRequestId.fetch_add(1);
    p.sendRank = sendRank;
    p.recvRank = recvRank;
    p.buffer = buffer;
    p.bytes = mpiTypeSize(dataType) * (size_t)count;
    p.type = messageType;
    if (isDeviceBuffer(buffer, loc)) {
        if (rcclUsable(recvRank)) {
            ncclComm_t comm;
            hipStream_t stream;
            {
                std::lock_guard<std::mutex> lock(rccl->mx);
                comm = rccl->comms.at(recvRank);
                stream = rccl->streams.at(recvRank);
                HIP_CHECK(hipSetDevice(rccl->devices.at(recvRank)));
            }
            RCCL_CHECK(ncclRecv(buffer, count, toNccl(dataType),
                                sendRank, comm, stream));
            hipEvent_t ev;
            HIP_CHECK(
              hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(ev, stream));
            rankState.deviceEvents[p.requestId] = ev;
            return p.requestId;
        }
        p.onDevice = true; // drained via devRecv at await time
    }
    rankState.pendingRecvs.push_back(p);
    return p.requestId;
}

void MpiWorld::awaitAsyncRequest(int requestId)
{
    // Stream-ordered RCCL request: wait on its event
    auto evIt = rankState.deviceEvents.find(requestId);
    if (evIt != rankState.deviceEvents.end()) {
        HIP_CHECK(hipEventSynchronize(evIt->second));
        (void)hipEventDestroy(evIt->second);
        rankState.deviceEvents.erase(evIt);
        return;
    }
    auto& pending = rankState.pendingRecvs;
    auto target = std::find_if(
      pending.begin(), pending.end(), [&](const PendingRecv& p) {
          return p.requestId == requestId;
      });
    if (target == pending.end()) {
        return; // isend request or already-awaited
    }
    if (!target->done) {
        // Drain earlier pending recvs on the same channel first so
        // message order per (sender, receiver, type) is preserved
        for (auto& p : pending) {
            if (p.done || p.sendRank != target->sendRank ||
                p.recvRank != target->recvRank || p.type != target->type) {
                continue;
            }
            if (p.onDevice) {
                devRecv(p.sendRank, p.recvRank, p.buffer, p.bytes,
                        p.type);
            } else {
                auto data =
                  hostRecv(p.sendRank, p.recvRank, p.bytes, p.type);
                std::memcpy(p.buffer, data.data(), data.size());
            }
            p.done = true;
            if (p.requestId == requestId) {
                break;
            }
        }
    }
    pending.erase(std::remove_if(pending.begin(),
                                 pending.end(),
                                 [&](const PendingRecv& p) {
                                     return p.requestId == requestId;
                                 }),
                  pending.end());
}

void MpiWorld::sendRecv(const uint8_t* sendBuffer,
                        int sendCount,
                        MpiDataType sendType,
                        int sendToRank,
                        uint8_t* recvBuffer,
                        int recvCount,
                        MpiDataType recvType,
                        int recvFromRank,
                        int thisRank)
{
    // Each buffer is probed on its own: a host pointer never reaches the
    // device plane and a device pointer never reaches a host memcpy
    bool sendOnDevice = isDeviceBuffer(sendBuffer, MpiBufferLoc::AUTO);
    bool recvOnDevice = isDeviceBuffer(recvBuffer, MpiBufferLoc::AUTO);
    if (sendOnDevice != recvOnDevice) {
        if (rcclUsable(thisRank)) {
            throw FaabricException(
              "sendRecv with one host and one device buffer is only "
              "supported on the PTP device plane");
        }
        // The PTP broker converts between host and device payloads, so
        // each side rides its own plane. Sends are buffered on both, so
        // send-then-recv cannot deadlock in a ring.
        size_t sendBytes = mpiTypeSize(sendType) * (size_t)sendCount;
        size_t recvBytes = mpiTypeSize(recvType) * (size_t)recvCount;
        if (sendOnDevice) {
            devSend(thisRank, sendToRank, sendBuffer, sendBytes,
                    MpiMessageType::SENDRECV);
        } else {
            hostSend(thisRank, sendToRank, sendBuffer, sendBytes,
                     MpiMessageType::SENDRECV);
        }
        if (recvOnDevice) {
            devRecv(recvFromRank, thisRank, recvBuffer, recvBytes,
                    MpiMessageType::SENDRECV);
        } else {
            auto data = hostRecv(recvFromRank, thisRank, recvBytes,
                                 MpiMessageType::SENDRECV);
            std::memcpy(recvBuffer, data.data(), data.size());
        }
        return;
    }
    if (sendOnDevice) {
        if (!rcclUsable(thisRank)) {
            // Buffered device sends never rendezvous, so send-then-recv
            // cannot deadlock in a ring
            devSend(thisRank, sendToRank, sendBuffer,
                    mpiTypeSize(sendType) * (size_t)sendCount,
                    MpiMessageType::SENDRECV);
            devRecv(recvFromRank, thisRank, recvBuffer,
                    mpiTypeSize(recvType) * (size_t)recvCount,
                    MpiMessageType::SENDRECV);
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        RCCL_CHECK(ncclGroupStart());
        RCCL_CHECK(ncclSend(sendBuffer,
                            sendCount,
                            toNccl(sendType),
                            sendToRank,
                            comm,
                            stream));
        RCCL_CHECK(ncclRecv(recvBuffer,
                            recvCount,
                            toNccl(recvType),
                            recvFromRank,
                            comm,
                            stream));
        RCCL_CHECK(ncclGroupEnd());
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    int req = irecv(recvFromRank,
                    thisRank,
                    recvBuffer,
                    recvType,
                    recvCount,
                    MpiMessageType::SENDRECV);
    send(thisRank,
         sendToRank,
         sendBuffer,
         sendType,
         sendCount,
         MpiMessageType::SENDRECV);
    awaitAsyncRequest(req);
}

// ------------------------- op_reduce ----------------------------------------

template<typename T>
static void opReduceLoop(MpiOp op, int count, const T* in, T* inout)
{
    switch (op) {
        case MpiOp::SUM:
            for (int i = 0; i < count; i++) {
                inout[i] += in[i];
            }
            break;
        case MpiOp::MAX:
            for (int i = 0; i < count; i++) {
                inout[i] = std::max(inout[i], in[i]);
            }
            break;
        case MpiOp::MIN:
            for (int i = 0; i < count; i++) {
                inout[i] = std::min(inout[i], in[i]);
            }
            break;
        case MpiOp::PROD:
            for (int i = 0; i < count; i++) {
                inout[i] *= in[i];
            }
            break;
    }
}

void MpiWorld::opReduceHost(MpiOp op,
                            MpiDataType type,
                            int count,
                            const uint8_t* in,
                            uint8_t* inout)
{
    switch (type) {
        case MpiDataType::INT32:
            opReduceLoop(op, count, (const int32_t*)in, (int32_t*)inout);
            break;
        case MpiDataType::INT64:
            opReduceLoop(op, count, (const int64_t*)in, (int64_t*)inout);
            break;
        case MpiDataType::UINT64:
            opReduceLoop(op, count, (const uint64_t*)in, (uint64_t*)inout);
            break;
        case MpiDataType::FLOAT:
            opReduceLoop(op, count, (const float*)in, (float*)inout);
            break;
        case MpiDataType::DOUBLE:
            opReduceLoop(op, count, (const double*)in, (double*)inout);
            break;
        case MpiDataType::BYTE:
            opReduceLoop(op, count, (const uint8_t*)in, (uint8_t*)inout);
            break;
    }
}

// ------------------------- collectives --------------------------------------

void MpiWorld::barrier(int thisRank)
{
    // All join at rank 0, rank 0 releases
    // (reference: src/mpi/MpiWorld.cpp:1753-1775)
    uint8_t token = 1;
    if (thisRank == 0) {
        for (int i = 1; i < size; i++) {
            hostRecv(i, 0, 1, MpiMessageType::BARRIER_JOIN);
        }
        for (int i = 1; i < size; i++) {
            hostSend(0, i, &token, 1, MpiMessageType::BARRIER_DONE);
        }
    } else {
        hostSend(thisRank, 0, &token, 1, MpiMessageType::BARRIER_JOIN);
        hostRecv(0, thisRank, 1, MpiMessageType::BARRIER_DONE);
    }
}

void MpiWorld::broadcast(int rootRank,
                         int thisRank,
                         uint8_t* buffer,
                         MpiDataType dataType,
                         int count,
                         MpiMessageType messageType,
                         MpiBufferLoc loc)
{
    if (size == 1 && isDeviceBuffer(buffer, loc)) {
        return; // broadcast to self is a no-op
    }
    if (isDeviceBuffer(buffer, loc)) {
        if (!rcclUsable(thisRank)) {
            deviceBroadcastFallback(rootRank, thisRank, buffer,
                                    mpiTypeSize(dataType) * (size_t)count,
                                    messageType);
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        RCCL_CHECK(ncclBroadcast(buffer,
                                 buffer,
                                 count,
                                 toNccl(dataType),
                                 rootRank,
                                 comm,
                                 stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // Two-level host plane: the root sends once per remote host (to its
    // local leader) plus to its own local ranks; leaders re-broadcast
    // locally (reference: src/mpi/MpiWorld.cpp:786-854). Collapses to
    // the flat fan-out when every rank has its own worker.
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    auto hostsMap = ranksPerHost();
    const std::string& rootHost = getHostForRank(rootRank);
    const std::string& myHost = getHostForRank(thisRank);
    if (thisRank == rootRank) {
        for (int r : hostsMap[rootHost]) {
            if (r != rootRank) {
                hostSend(rootRank, r, buffer, bytes, messageType);
            }
        }
        for (auto& [h, ranks] : hostsMap) {
            if (h != rootHost) {
                hostSend(rootRank, ranks[0], buffer, bytes, messageType);
            }
        }
    } else if (myHost != rootHost && thisRank == hostsMap[myHost][0]) {
        // Local leader: take the root's copy, fan out on this host
        auto data = hostRecv(rootRank, thisRank, bytes, messageType);
        std::memcpy(buffer, data.data(), data.size());
        for (int r : hostsMap[myHost]) {
            if (r != thisRank) {
                hostSend(thisRank, r, buffer, bytes, messageType);
            }
        }
    } else {
        int from = myHost == rootHost ? rootRank : hostsMap[myHost][0];
        auto data = hostRecv(from, thisRank, bytes, messageType);
        std::memcpy(buffer, data.data(), data.size());
    }
}

void MpiWorld::scatter(int rootRank,
                       int thisRank,
                       const uint8_t* sendBuffer,
                       uint8_t* recvBuffer,
                       MpiDataType dataType,
                       int count,
                       MpiBufferLoc loc)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    // Only the root's sendBuffer is significant, so every rank probes the
    // buffer it always has
    if (isDeviceBuffer(recvBuffer, loc)) {
        // PTP device plane on every deployment (it works with or without
        // RCCL): remote chunks leave straight from sendBuffer + i*bytes
        if (thisRank != rootRank) {
            devRecv(rootRank, thisRank, recvBuffer, bytes,
                    MpiMessageType::SCATTER);
            return;
        }
        for (int i = 0; i < size; i++) {
            const uint8_t* chunk = sendBuffer + (size_t)i * bytes;
            if (i != rootRank) {
                devSend(rootRank, i, chunk, bytes, MpiMessageType::SCATTER);
            } else if (recvBuffer != chunk && bytes > 0) {
                hipStream_t s = (hipStream_t)fallbackStream();
                HIP_CHECK(famCopyBuffer(chunk, recvBuffer, bytes, s));
                HIP_CHECK(hipStreamSynchronize(s));
            }
        }
        return;
    }
    if (thisRank == rootRank) {
        for (int i = 0; i < size; i++) {
            const uint8_t* chunk = sendBuffer + (size_t)i * bytes;
            if (i == rootRank) {
                if (recvBuffer != chunk) {
                    std::memcpy(recvBuffer, chunk, bytes);
                }
            } else {
                hostSend(rootRank, i, chunk, bytes,
                         MpiMessageType::SCATTER);
            }
        }
    } else {
        auto data =
          hostRecv(rootRank, thisRank, bytes, MpiMessageType::SCATTER);
        std::memcpy(recvBuffer, data.data(), data.size());
    }
}

void MpiWorld::gather(int thisRank,
                      int rootRank,
                      const uint8_t* sendBuffer,
                      uint8_t* recvBuffer,
                      MpiDataType dataType,
                      int count,
                      MpiBufferLoc loc)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    // Only the root's recvBuffer is significant, so every rank probes the
    // buffer it always has
    if (isDeviceBuffer(sendBuffer, loc)) {
        // PTP device plane on every deployment (it works with or without
        // RCCL): remote chunks land straight in recvBuffer + i*bytes
        if (thisRank != rootRank) {
            devSend(thisRank, rootRank, sendBuffer, bytes,
                    MpiMessageType::GATHER);
            return;
        }
        uint8_t* own = recvBuffer + (size_t)rootRank * bytes;
        if (own != sendBuffer && bytes > 0) {
            hipStream_t s = (hipStream_t)fallbackStream();
            HIP_CHECK(famCopyBuffer(sendBuffer, own, bytes, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        for (int i = 0; i < size; i++) {
            if (i != rootRank) {
                devRecv(i, rootRank, recvBuffer + (size_t)i * bytes, bytes,
                        MpiMessageType::GATHER);
            }
        }
        return;
    }
    // Two-level host plane: leaders gather their host's chunks in rank
    // order and send one batched buffer to the root, which unpacks by
    // the shared ranksPerHost layout (reference: :917-1080)
    auto hostsMap = ranksPerHost();
    const std::string& rootHost = getHostForRank(rootRank);
    const std::string& myHost = getHostForRank(thisRank);
    if (thisRank == rootRank) {
        uint8_t* own = recvBuffer + (size_t)rootRank * bytes;
        if (own != sendBuffer) {
            std::memcpy(own, sendBuffer, bytes);
        }
        for (int r : hostsMap[rootHost]) {
            if (r == rootRank) {
                continue;
            }
            auto data =
              hostRecv(r, rootRank, bytes, MpiMessageType::GATHER);
            std::memcpy(recvBuffer + (size_t)r * bytes, data.data(),
                        data.size());
        }
        for (auto& [h, ranks] : hostsMap) {
            if (h == rootHost) {
                continue;
            }
            auto batch = hostRecv(ranks[0], rootRank,
                                  bytes * ranks.size(),
                                  MpiMessageType::GATHER);
            for (size_t i = 0; i < ranks.size(); i++) {
                std::memcpy(recvBuffer + (size_t)ranks[i] * bytes,
                            batch.data() + i * bytes,
                            bytes);
            }
        }
    } else if (myHost == rootHost) {
        hostSend(thisRank, rootRank, sendBuffer, bytes,
                 MpiMessageType::GATHER);
    } else if (thisRank == hostsMap[myHost][0]) {
        auto& ranks = hostsMap[myHost];
        std::vector<uint8_t> batch(bytes * ranks.size());
        for (size_t i = 0; i < ranks.size(); i++) {
            if (ranks[i] == thisRank) {
                std::memcpy(batch.data() + i * bytes, sendBuffer, bytes);
            } else {
                auto data = hostRecv(ranks[i], thisRank, bytes,
                                     MpiMessageType::GATHER);
                std::memcpy(batch.data() + i * bytes, data.data(),
                            data.size());
            }
        }
        hostSend(thisRank, rootRank, batch.data(), batch.size(),
                 MpiMessageType::GATHER);
    } else {
        hostSend(thisRank, hostsMap[myHost][0], sendBuffer, bytes,
                 MpiMessageType::GATHER);
    }
}

void MpiWorld::allGather(int thisRank,
                         const uint8_t* sendBuffer,
                         uint8_t* recvBuffer,
                         MpiDataType dataType,
                         int count,
                         MpiBufferLoc loc)
{
    if (size == 1 && isDeviceBuffer(recvBuffer, loc)) {
        size_t bytes = mpiTypeSize(dataType) * (size_t)count;
        if (recvBuffer != sendBuffer) {
            // NT copy kernel beats hipMemcpy D2D for HBM buffers; sync
            // so the collective keeps blocking semantics (honest timings)
            HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes,
                                    nullptr));
            HIP_CHECK(hipStreamSynchronize(nullptr));
        }
        return;
    }
    if (isDeviceBuffer(recvBuffer, loc)) {
        if (!rcclUsable(thisRank)) {
            // Gather at 0 (each rank's chunk lands straight in 0's
            // recvBuffer slot), then broadcast the full device buffer
            size_t bytes = mpiTypeSize(dataType) * (size_t)count;
            if (thisRank == 0) {
                hipStream_t s = (hipStream_t)fallbackStream();
                if (recvBuffer != sendBuffer) {
                    HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer,
                                            bytes, s));
                    HIP_CHECK(hipStreamSynchronize(s));
                }
                for (int i = 1; i < size; i++) {
                    devRecv(i, 0, recvBuffer + (size_t)i * bytes, bytes,
                            MpiMessageType::ALLGATHER);
                }
            } else {
                devSend(thisRank, 0, sendBuffer, bytes,
                        MpiMessageType::ALLGATHER);
            }
            deviceBroadcastFallback(0, thisRank, recvBuffer,
                                    bytes * (size_t)size,
                                    MpiMessageType::ALLGATHER);
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        RCCL_CHECK(ncclAllGather(
          sendBuffer, recvBuffer, count, toNccl(dataType), comm, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // gather at 0, then broadcast the full buffer (reference: :1082-1111)
    gather(thisRank, 0, sendBuffer, recvBuffer, dataType, count,
           MpiBufferLoc::HOST);
    broadcast(0,
              thisRank,
              recvBuffer,
              dataType,
              count * size,
              MpiMessageType::ALLGATHER,
              MpiBufferLoc::HOST);
}

void MpiWorld::reduce(int thisRank,
                      int rootRank,
                      const uint8_t* sendBuffer,
                      uint8_t* recvBuffer,
                      MpiDataType dataType,
                      int count,
                      MpiOp op,
                      MpiBufferLoc loc)
{
    if (size == 1 && isDeviceBuffer(sendBuffer, loc)) {
        size_t bytes = mpiTypeSize(dataType) * (size_t)count;
        if (recvBuffer != sendBuffer) {
            // NT copy kernel beats hipMemcpy D2D for HBM buffers; sync
            // so the collective keeps blocking semantics (honest timings)
            HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes,
                                    nullptr));
            HIP_CHECK(hipStreamSynchronize(nullptr));
        }
        return;
    }
    if (isDeviceBuffer(sendBuffer, loc)) {
        if (!rcclUsable(thisRank)) {
            deviceReduceFallback(thisRank, rootRank, sendBuffer,
                                 recvBuffer, dataType, count, op);
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        RCCL_CHECK(ncclReduce(sendBuffer,
                              recvBuffer,
                              count,
                              toNccl(dataType),
                              toNcclOp(op),
                              rootRank,
                              comm,
                              stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // Two-level host plane: remote hosts' ranks reduce at their local
    // leader, leaders send one partial to the root (reference:
    // src/mpi/MpiWorld.cpp:1127-1249)
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    auto hostsMap = ranksPerHost();
    const std::string& rootHost = getHostForRank(rootRank);
    const std::string& myHost = getHostForRank(thisRank);
    if (thisRank == rootRank) {
        if (recvBuffer != sendBuffer) {
            std::memcpy(recvBuffer, sendBuffer, bytes);
        }
        for (int r : hostsMap[rootHost]) {
            if (r == rootRank) {
                continue;
            }
            auto data =
              hostRecv(r, rootRank, bytes, MpiMessageType::REDUCE);
            opReduceHost(op, dataType, count, data.data(), recvBuffer);
        }
        for (auto& [h, ranks] : hostsMap) {
            if (h == rootHost) {
                continue;
            }
            auto data = hostRecv(ranks[0], rootRank, bytes,
                                 MpiMessageType::REDUCE);
            opReduceHost(op, dataType, count, data.data(), recvBuffer);
        }
    } else if (myHost == rootHost) {
        hostSend(thisRank, rootRank, sendBuffer, bytes,
                 MpiMessageType::REDUCE);
    } else if (thisRank == hostsMap[myHost][0]) {
        // Local leader: fold this host's ranks, ship one partial
        std::vector<uint8_t> partial(sendBuffer, sendBuffer + bytes);
        for (int r : hostsMap[myHost]) {
            if (r == thisRank) {
                continue;
            }
            auto data =
              hostRecv(r, thisRank, bytes, MpiMessageType::REDUCE);
            opReduceHost(op, dataType, count, data.data(),
                         partial.data());
        }
        hostSend(thisRank, rootRank, partial.data(), bytes,
                 MpiMessageType::REDUCE);
    } else {
        hostSend(thisRank, hostsMap[myHost][0], sendBuffer, bytes,
                 MpiMessageType::REDUCE);
    }
}

void MpiWorld::allReduce(int thisRank,
                         const uint8_t* sendBuffer,
                         uint8_t* recvBuffer,
                         MpiDataType dataType,
                         int count,
                         MpiOp op,
                         MpiBufferLoc loc)
{
    if (size == 1 && isDeviceBuffer(sendBuffer, loc)) {
        // Single-rank collective = local copy; skip the RCCL machinery
        size_t bytes = mpiTypeSize(dataType) * (size_t)count;
        if (recvBuffer != sendBuffer) {
            // NT copy kernel beats hipMemcpy D2D for HBM buffers; sync
            // so the collective keeps blocking semantics (honest timings)
            HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes,
                                    nullptr));
            HIP_CHECK(hipStreamSynchronize(nullptr));
        }
        return;
    }
    if (isDeviceBuffer(sendBuffer, loc)) {
        if (!rcclUsable(thisRank)) {
            // reduce to 0 then broadcast, all on the device plane
            deviceReduceFallback(thisRank, 0, sendBuffer, recvBuffer,
                                 dataType, count, op);
            deviceBroadcastFallback(0, thisRank, recvBuffer,
                                    mpiTypeSize(dataType) * (size_t)count,
                                    MpiMessageType::ALLREDUCE);
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        RCCL_CHECK(ncclAllReduce(sendBuffer,
                                 recvBuffer,
                                 count,
                                 toNccl(dataType),
                                 toNcclOp(op),
                                 comm,
                                 stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // reduce to 0 then broadcast (reference: :1251-1264)
    reduce(thisRank, 0, sendBuffer, recvBuffer, dataType, count, op,
           MpiBufferLoc::HOST);
    broadcast(0,
              thisRank,
              recvBuffer,
              dataType,
              count,
              MpiMessageType::ALLREDUCE,
              MpiBufferLoc::HOST);
}

void MpiWorld::allToAll(int thisRank,
                        const uint8_t* sendBuffer,
                        uint8_t* recvBuffer,
                        MpiDataType dataType,
                        int count,
                        MpiBufferLoc loc)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    if (size == 1 && isDeviceBuffer(sendBuffer, loc)) {
        if (recvBuffer != sendBuffer) {
            // NT copy kernel beats hipMemcpy D2D for HBM buffers; sync
            // so the collective keeps blocking semantics (honest timings)
            HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes,
                                    nullptr));
            HIP_CHECK(hipStreamSynchronize(nullptr));
        }
        return;
    }
    if (isDeviceBuffer(sendBuffer, loc)) {
        if (!rcclUsable(thisRank)) {
            // Direct pairwise exchange; buffered sends first, then recvs
            hipStream_t s = (hipStream_t)fallbackStream();
            for (int i = 0; i < size; i++) {
                const uint8_t* chunk = sendBuffer + (size_t)i * bytes;
                if (i == thisRank) {
                    uint8_t* dst = recvBuffer + (size_t)i * bytes;
                    if (dst != chunk) {
                        HIP_CHECK(famCopyBuffer(chunk, dst, bytes, s));
                        HIP_CHECK(hipStreamSynchronize(s));
                    }
                } else {
                    devSend(thisRank, i, chunk, bytes,
                            MpiMessageType::ALLTOALL);
                }
            }
            for (int i = 0; i < size; i++) {
                if (i == thisRank) {
                    continue;
                }
                devRecv(i, thisRank, recvBuffer + (size_t)i * bytes,
                        bytes, MpiMessageType::ALLTOALL);
            }
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        // Pairwise xGMI exchange under one group
        RCCL_CHECK(ncclGroupStart());
        for (int i = 0; i < size; i++) {
            RCCL_CHECK(ncclSend(sendBuffer + (size_t)i * bytes,
                                count,
                                toNccl(dataType),
                                i,
                                comm,
                                stream));
            RCCL_CHECK(ncclRecv(recvBuffer + (size_t)i * bytes,
                                count,
                                toNccl(dataType),
                                i,
                                comm,
                                stream));
        }
        RCCL_CHECK(ncclGroupEnd());
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // Direct N² exchange (reference: :1433-1484)
    for (int i = 0; i < size; i++) {
        const uint8_t* chunk = sendBuffer + (size_t)i * bytes;
        if (i == thisRank) {
            std::memcpy(recvBuffer + (size_t)i * bytes, chunk, bytes);
        } else {
            hostSend(thisRank, i, chunk, bytes, MpiMessageType::ALLTOALL);
        }
    }
    for (int i = 0; i < size; i++) {
        if (i == thisRank) {
            continue;
        }
        auto data = hostRecv(i, thisRank, bytes, MpiMessageType::ALLTOALL);
        std::memcpy(recvBuffer + (size_t)i * bytes,
                    data.data(),
                    data.size());
    }
}

void MpiWorld::scan(int thisRank,
                    const uint8_t* sendBuffer,
                    uint8_t* recvBuffer,
                    MpiDataType dataType,
                    int count,
                    MpiOp op,
                    MpiBufferLoc loc)
{
    size_t bytes = mpiTypeSize(dataType) * (size_t)count;
    if (isDeviceBuffer(sendBuffer, loc)) {
        if (!rcclUsable(thisRank)) {
            // Linear chain over the PTP device plane with the same
            // fused elementwise combine
            if (bytes == 0) {
                return; // same count on every rank: no chain to run
            }
            hipStream_t s = (hipStream_t)fallbackStream();
            if (recvBuffer != sendBuffer) {
                HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes,
                                        s));
                HIP_CHECK(hipStreamSynchronize(s));
            }
            if (thisRank > 0) {
                uint8_t* tmp = nullptr;
                HIP_CHECK(hipMallocAsync((void**)&tmp, bytes, s));
                devRecv(thisRank - 1, thisRank, tmp, bytes,
                        MpiMessageType::SCAN);
                deviceElementwiseOp(recvBuffer, tmp, (uint64_t)count,
                                    (int)dataType, (int)op, s);
                HIP_CHECK(hipFreeAsync(tmp, s));
                HIP_CHECK(hipStreamSynchronize(s));
            }
            if (thisRank < size - 1) {
                devSend(thisRank, thisRank + 1, recvBuffer, bytes,
                        MpiMessageType::SCAN);
            }
            return;
        }
        // Device chain: RCCL p2p hop + fused elementwise combine on the
        // GPU (the SURVEY worklist's "GPU prefix + p2p chain" mapping for
        // the reference's linear scan, src/mpi/MpiWorld.cpp:1390-1432)
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        if (recvBuffer != sendBuffer) {
            HIP_CHECK(famCopyBuffer(sendBuffer, recvBuffer, bytes, stream));
        }
        if (thisRank > 0) {
            uint8_t* tmp = nullptr;
            HIP_CHECK(hipMallocAsync((void**)&tmp, bytes, stream));
            RCCL_CHECK(ncclRecv(tmp, count, toNccl(dataType), thisRank - 1,
                                comm, stream));
            HIP_CHECK(famElementwiseOp(recvBuffer, tmp, (uint64_t)count,
                                       (int)dataType, (int)op, stream));
            HIP_CHECK(hipFreeAsync(tmp, stream));
        }
        if (thisRank < size - 1) {
            RCCL_CHECK(ncclSend(recvBuffer, count, toNccl(dataType),
                                thisRank + 1, comm, stream));
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // Inclusive prefix along a linear chain (reference: :1390-1432)
    std::memcpy(recvBuffer, sendBuffer, bytes);
    if (thisRank > 0) {
        auto data =
          hostRecv(thisRank - 1, thisRank, bytes, MpiMessageType::SCAN);
        opReduceHost(op, dataType, count, data.data(), recvBuffer);
    }
    if (thisRank < size - 1) {
        hostSend(thisRank, thisRank + 1, recvBuffer, bytes,
                 MpiMessageType::SCAN);
    }
}

void MpiWorld::reduceScatter(int thisRank,
                             const uint8_t* sendBuffer,
                             uint8_t* recvBuffer,
                             MpiDataType dataType,
                             int recvCount,
                             MpiOp op,
                             MpiBufferLoc loc)
{
    if (isDeviceBuffer(sendBuffer, loc)) {
        if (!rcclUsable(thisRank)) {
            // Reduce the full buffer at 0, then scatter each rank its
            // slice over the device plane
            size_t sliceBytes = mpiTypeSize(dataType) * (size_t)recvCount;
            size_t fullBytes = sliceBytes * (size_t)size;
            if (sliceBytes == 0) {
                return; // same count on every rank: no slice to send
            }
            hipStream_t s = (hipStream_t)fallbackStream();
            if (thisRank == 0) {
                uint8_t* full = nullptr;
                HIP_CHECK(hipMallocAsync((void**)&full, fullBytes, s));
                HIP_CHECK(hipStreamSynchronize(s));
                deviceReduceFallback(0, 0, sendBuffer, full, dataType,
                                     recvCount * size, op);
                HIP_CHECK(famCopyBuffer(full, recvBuffer, sliceBytes, s));
                HIP_CHECK(hipStreamSynchronize(s));
                for (int i = 1; i < size; i++) {
                    devSend(0, i, full + (size_t)i * sliceBytes,
                            sliceBytes, MpiMessageType::SCATTER);
                }
                HIP_CHECK(hipFreeAsync(full, s));
                HIP_CHECK(hipStreamSynchronize(s));
            } else {
                deviceReduceFallback(thisRank, 0, sendBuffer, nullptr,
                                     dataType, recvCount * size, op);
                devRecv(0, thisRank, recvBuffer, sliceBytes,
                        MpiMessageType::SCATTER);
            }
            return;
        }
        ncclComm_t comm;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(rccl->mx);
            comm = rccl->comms.at(thisRank);
            stream = rccl->streams.at(thisRank);
            HIP_CHECK(hipSetDevice(rccl->devices.at(thisRank)));
        }
        RCCL_CHECK(ncclReduceScatter(sendBuffer,
                                     recvBuffer,
                                     recvCount,
                                     toNccl(dataType),
                                     toNcclOp(op),
                                     comm,
                                     stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    // allreduce then slice (host path; the reference stubs this call)
    size_t bytes = mpiTypeSize(dataType) * (size_t)recvCount;
    std::vector<uint8_t> full((size_t)size * bytes);
    allReduce(thisRank,
              sendBuffer,
              full.data(),
              dataType,
              recvCount * size,
              op,
              MpiBufferLoc::HOST);
    std::memcpy(recvBuffer, full.data() + (size_t)thisRank * bytes, bytes);
}

double MpiWorld::getWTime()
{
    return getSecondsSinceEpoch();
}

void MpiWorld::recordMsgCount(int sendRank,
                              int recvRank,
                              MpiMessageType type)
{
    // Only recorded when the executing message asks for an exec graph
    if (!ExecutorContext::isSet()) {
        return;
    }
    Message& msg = ExecutorContext::get().getMsg();
    if (!msg.recordExecGraph) {
        return;
    }
    std::lock_guard<std::mutex> lock(statsMx);
    auto& counts = msgCounts[sendRank];
    counts["mpi-msgcount-torank-" + std::to_string(recvRank)] += 1;
    counts["mpi-msgtype-" + std::to_string((int)type) + "-torank-" +
           std::to_string(recvRank)] += 1;
}

std::map<std::string, int32_t> MpiWorld::getMsgCountDetails(int rank)
{
    std::lock_guard<std::mutex> lock(statsMx);
    return msgCounts[rank];
}

void MpiWorld::refreshGroupFromMsg(Message& msg)
{
    if (msg.groupId == 0) {
        return;
    }
    {
        std::lock_guard<std::mutex> lock(worldMx);
        if (msg.groupId == groupId) {
            return;
        }
    }
    // New scheduling event renamed the group: wait for the new group's
    // mappings (the planner distributes them with the dispatch), then
    // adopt the new placement exactly like a stayed rank does
    getPointToPointBroker().waitForMappingsOnThisHost(msg.groupId);
    prepareMigration(msg.mpiRank);
}

void MpiWorld::prepareMigration(int thisRank)
{
    // No pending async requests may be in flight
    // (reference: src/mpi/MpiWorld.cpp:2095-2132)
    if (!rankState.pendingRecvs.empty() ||
        !rankState.deviceEvents.empty()) {
        throw FaabricException(
          "cannot migrate with pending async MPI requests");
    }
    // Refresh the placement from the planner's new decision
    auto decision = getPlannerClient().getSchedulingDecision(appId);
    if (decision.nFunctions > 0) {
        groupId = decision.groupId;
        std::lock_guard<std::mutex> lock(worldMx);
        rankHosts.assign(size, "");
        for (int i = 0; i < decision.nFunctions; i++) {
            if (decision.groupIdxs[i] < size) {
                rankHosts[decision.groupIdxs[i]] = decision.hosts[i];
            }
        }
    }
    // Device-side communicators must be rebuilt after migration (like the
    // reference clears TLS sockets)
    std::lock_guard<std::mutex> lock(worldMx);
    rccl.reset();
}

// ------------------------- registry / context -------------------------------

MpiWorldRegistry& MpiWorldRegistry::get()
{
    static MpiWorldRegistry reg;
    return reg;
}

MpiWorld& MpiWorldRegistry::createWorld(Message& msg, int worldId)
{
    std::lock_guard<std::mutex> lock(mx);
    if (worlds.count(worldId) > 0) {
        throw FaabricException("MPI world already exists: " +
                               std::to_string(worldId));
    }
    auto world = std::make_shared<MpiWorld>();
    worlds[worldId] = world;
    world->create(msg, worldId, msg.mpiWorldSize);
    return *world;
}

MpiWorld& MpiWorldRegistry::getOrInitialiseWorld(Message& msg)
{
    std::shared_ptr<MpiWorld> world;
    bool existed = false;
    {
        std::lock_guard<std::mutex> lock(mx);
        auto it = worlds.find(msg.mpiWorldId);
        if (it == worlds.end()) {
            world = std::make_shared<MpiWorld>();
            worlds[msg.mpiWorldId] = world;
            world->initialiseFromMsg(msg);
        } else {
            world = it->second;
            existed = true;
        }
    }
    if (existed) {
        // A migrated rank can land on a host whose world still carries
        // the pre-migration group id (stayed ranks adopt the new one on
        // their own schedule); refresh before any collective touches
        // stale channels — otherwise this rank blocks forever on the
        // old group while its peers talk on the new one
        world->refreshGroupFromMsg(msg);
    }
    world->initialiseRankFromMsg(msg);
    return *world;
}

MpiWorld& MpiWorldRegistry::getWorld(int worldId)
{
    std::lock_guard<std::mutex> lock(mx);
    auto it = worlds.find(worldId);
    if (it == worlds.end()) {
        throw FaabricException("MPI world not found: " +
                               std::to_string(worldId));
    }
    return *it->second;
}

bool MpiWorldRegistry::worldExists(int worldId)
{
    std::lock_guard<std::mutex> lock(mx);
    return worlds.count(worldId) > 0;
}

void MpiWorldRegistry::clearWorld(int worldId)
{
    std::lock_guard<std::mutex> lock(mx);
    worlds.erase(worldId);
}

void MpiWorldRegistry::clear()
{
    std::lock_guard<std::mutex> lock(mx);
    worlds.clear();
}

MpiContext::MpiContext() = default;

static thread_local MpiContext threadMpiContext;

MpiContext& getMpiContext()
{
    return threadMpiContext;
}

int MpiContext::createWorld(Message& msg)
{
    // (reference: src/mpi/MpiContext.cpp:14)
    if (msg.mpiRank > 0) {
        throw FaabricException("createWorld called by non-zero rank");
    }
    int worldId = msg.mpiWorldId != 0 ? msg.mpiWorldId : generateGidInt32();
    msg.mpiWorldId = worldId;
    // A migrated or unfrozen rank 0 re-enters with a snapshotKey (and the
    // world may already live on this host): JOIN the existing cluster-wide
    // world instead of re-creating it (reference: re-entry goes through
    // getOrInitialiseWorld, src/mpi/MpiWorldRegistry.cpp)
    if (!msg.snapshotKey.empty() ||
        MpiWorldRegistry::get().worldExists(worldId)) {
        MpiWorldRegistry::get().getOrInitialiseWorld(msg);
    } else {
        MpiWorldRegistry::get().createWorld(msg, worldId);
    }
    isMpi = true;
    rank = 0;
    this->worldId = worldId;
    return worldId;
}

void MpiContext::joinWorld(Message& msg)
{
    if (!msg.isMpi) {
        throw FaabricException("joinWorld on non-MPI message");
    }
    isMpi = true;
    worldId = msg.mpiWorldId;
    rank = msg.mpiRank;
    MpiWorldRegistry::get().getOrInitialiseWorld(msg);
}

MpiWorld& MpiContext::getWorld()
{
    return MpiWorldRegistry::get().getWorld(worldId);
}

} // namespace faabricamd

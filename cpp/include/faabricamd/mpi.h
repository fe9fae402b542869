// MPI worlds on MI355X: one rank per GPU, collectives on RCCL over xGMI.
//
// MI355X-native re-design of the reference MPI subsystem (reference:
// include/faabric/mpi/MpiWorld.h:35-283, MpiWorldRegistry.h:7-28,
// MpiContext.h:7-27, src/mpi/MpiWorld.cpp). Differences by design:
//  - HOST buffers ride the point-to-point broker (in-process queues
//    locally, framed TCP remotely) instead of a bespoke raw-TCP full mesh:
//    the host path is the control/correctness path on this target
//  - DEVICE (HBM) buffers use an RCCL communicator per world — the
//    reference's two-level leader collectives collapse into RCCL's
//    multi-ring xGMI schedules; the communicator is
//    bootstrapped by broadcasting rank 0's ncclUniqueId over the broker
//    (replacing the reference's full-mesh TCP handshake :1789-1935)
//  - op_reduce CPU loops stay for host buffers; on device RCCL reduces
//    in-kernel, and scan uses a p2p ring with a gfx950 elementwise kernel
#pragma once

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "faabricamd/messages.h"
#include "faabricamd/scheduling.h"

namespace faabricamd {

// World size cap from the PTP channel packing (mpi channel namespace)
inline constexpr int MAX_MPI_WORLD_SIZE = 1024;

enum class MpiMessageType : int32_t
{
    NORMAL = 0,
    BARRIER_JOIN = 1,
    BARRIER_DONE = 2,
    SCATTER = 3,
    GATHER = 4,
    ALLGATHER = 5,
    REDUCE = 6,
    SCAN = 7,
    ALLREDUCE = 8,
    ALLTOALL = 9,
    SENDRECV = 11,
    BROADCAST = 12,
    HANDSHAKE = 14, // RCCL uniqueId bootstrap rides the host plane
};

enum class MpiDataType : int32_t
{
    INT32 = 0,
    INT64 = 1,
    UINT64 = 2,
    FLOAT = 3,
    DOUBLE = 4,
    BYTE = 5,
};
size_t mpiTypeSize(MpiDataType t);

enum class MpiOp : int32_t
{
    SUM = 0,
    MAX = 1,
    MIN = 2,
    PROD = 3,
};

// Where a buffer lives; DEVICE pointers go through RCCL
enum class MpiBufferLoc : int32_t
{
    HOST = 0,
    DEVICE = 1,
    AUTO = 2, // probe with hipPointerGetAttributes
};

struct MpiRankState; // thread-local per-rank state (async requests etc.)

class MpiWorld
{
  public:
    MpiWorld();
    ~MpiWorld();

    // Rank 0 creates the world: the other size-1 ranks are dispatched as a
    // SCALE_CHANGE batch consuming the planner's preloaded gang decision
    // (reference: src/mpi/MpiWorld.cpp:157-226)
    void create(Message& call, int newId, int newSize);

    // Per-host init for joining ranks (reference: :270-283)
    void initialiseFromMsg(Message& msg);
    // Per-rank (thread-local) init (reference: :287-300)
    void initialiseRankFromMsg(Message& msg);

    std::string getHostForRank(int rank);
    std::map<std::string, std::vector<int>> ranksPerHost();
    const std::string& getUser() const { return user; }
    const std::string& getFunction() const { return function; }
    int getId() const { return id; }
    int getSize() const { return size; }

    bool destroy();
    // Returns true when this was the last local rank (world reclaimable)
    bool rankFinished(int rank); // true when no local ranks remain

    // --- cartesian topology (reference: :369-543) ---
    // N-dim row-major periodic grids; dims stored on the world the first
    // time the app supplies them (Cart_create or Cart_get), defaulting to
    // a 1-D {size} layout like the reference's pre-Cart state.
    void setCartesianDims(int ndims, const int* dims);
    void getCartesianRank(int rank,
                          int maxDims,
                          const int* dims,
                          int* periods,
                          int* coords);
    // Cart_get form: outputs the stored dims + this rank's coords
    void getCartesianGrid(int rank,
                          int maxDims,
                          int* dims,
                          int* periods,
                          int* coords);
    void getRankFromCoords(int* rank, int* coords);
    void shiftCartesianCoords(int rank,
                              int direction,
                              int disp,
                              int* source,
                              int* destination);

    // --- point-to-point ---
    void send(int sendRank,
              int recvRank,
              const uint8_t* buffer,
              MpiDataType dataType,
              int count,
              MpiMessageType messageType = MpiMessageType::NORMAL,
              MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void recv(int sendRank,
              int recvRank,
              uint8_t* buffer,
              MpiDataType dataType,
              int count,
              MpiMessageType messageType = MpiMessageType::NORMAL,
              MpiBufferLoc loc = MpiBufferLoc::AUTO);
    // Async p2p. Host sends are buffered-eager (complete immediately,
    // reference: src/mpi/MpiWorld.cpp:544-557); device sends/recvs on
    // the RCCL plane enqueue on the rank stream with a hipEvent per
    // request — awaitAsyncRequest waits on the event, isend never syncs
    int isend(int sendRank,
              int recvRank,
              const uint8_t* buffer,
              MpiDataType dataType,
              int count,
              MpiMessageType messageType = MpiMessageType::NORMAL,
              MpiBufferLoc loc = MpiBufferLoc::AUTO);
    int irecv(int sendRank,
              int recvRank,
              uint8_t* buffer,
              MpiDataType dataType,
              int count,
              MpiMessageType messageType = MpiMessageType::NORMAL,
              MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void awaitAsyncRequest(int requestId);
    void sendRecv(const uint8_t* sendBuffer,
                  int sendCount,
                  MpiDataType sendType,
                  int sendToRank,
                  uint8_t* recvBuffer,
                  int recvCount,
                  MpiDataType recvType,
                  int recvFromRank,
                  int thisRank);

    // --- collectives ---
    void barrier(int thisRank);
    void broadcast(int rootRank,
                   int thisRank,
                   uint8_t* buffer,
                   MpiDataType dataType,
                   int count,
                   MpiMessageType messageType = MpiMessageType::BROADCAST,
                   MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void scatter(int rootRank,
                 int thisRank,
                 const uint8_t* sendBuffer,
                 uint8_t* recvBuffer,
                 MpiDataType dataType,
                 int count,
                 MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void gather(int thisRank,
                int rootRank,
                const uint8_t* sendBuffer,
                uint8_t* recvBuffer,
                MpiDataType dataType,
                int count,
                MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void allGather(int thisRank,
                   const uint8_t* sendBuffer,
                   uint8_t* recvBuffer,
                   MpiDataType dataType,
                   int count,
                   MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void reduce(int thisRank,
                int rootRank,
                const uint8_t* sendBuffer,
                uint8_t* recvBuffer,
                MpiDataType dataType,
                int count,
                MpiOp op,
                MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void allReduce(int thisRank,
                   const uint8_t* sendBuffer,
                   uint8_t* recvBuffer,
                   MpiDataType dataType,
                   int count,
                   MpiOp op,
                   MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void allToAll(int thisRank,
                  const uint8_t* sendBuffer,
                  uint8_t* recvBuffer,
                  MpiDataType dataType,
                  int count,
                  MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void scan(int thisRank,
              const uint8_t* sendBuffer,
              uint8_t* recvBuffer,
              MpiDataType dataType,
              int count,
              MpiOp op,
              MpiBufferLoc loc = MpiBufferLoc::AUTO);
    void reduceScatter(int thisRank,
                       const uint8_t* sendBuffer,
                       uint8_t* recvBuffer,
                       MpiDataType dataType,
                       int recvCount,
                       MpiOp op,
                       MpiBufferLoc loc = MpiBufferLoc::AUTO);

    double getWTime();

    // Per-rank exec-graph message counters
    // (reference: mpi/MpiWorld.h:13-18)
    void recordMsgCount(int sendRank, int recvRank, MpiMessageType type);
    std::map<std::string, int32_t> getMsgCountDetails(int rank);

    // Migration support (reference: :2095-2132)
    void prepareMigration(int thisRank);

    // Adopt a newer group id carried by a (re-)joining rank's message
    // (migrated ranks can re-enter before stayed ranks refresh)
    void refreshGroupFromMsg(Message& msg);

    // The RCCL communicator for this world's local rank (GPU path);
    // created lazily on first device-buffer collective
    void* getRcclComm(int rank);
    void* getRankStream(int rank);

    int32_t getGroupId() const { return groupId; }

  private:
    int id = 0;
    int size = 0;
    int32_t appId = 0;
    int32_t groupId = 0;
    std::string user;
    std::string function;
    std::string thisHost;

    std::mutex worldMx;
    std::vector<std::string> rankHosts;
    std::vector<int> localRanks;

    // Cartesian grid dims (row-major, periodic); empty = 1-D {size}
    std::mutex cartMx;
    std::vector<int> cartDims;

    // Exec-graph counters: rank → (peer,type) counts
    std::mutex statsMx;
    std::map<int, std::map<std::string, int32_t>> msgCounts;

    // --- host data plane helpers ---
    void hostSend(int sendRank,
                  int recvRank,
                  const uint8_t* buffer,
                  size_t bytes,
                  MpiMessageType messageType);
    std::vector<uint8_t> hostRecv(int sendRank,
                                  int recvRank,
                                  size_t expectedBytes,
                                  MpiMessageType messageType);

    // --- device (RCCL) data plane ---
    struct RcclState;
    std::shared_ptr<RcclState> rccl;
    void ensureRcclComm(int rank);
    bool isDeviceBuffer(const void* ptr, MpiBufferLoc loc);

    // --- device fallback plane (PTP/HIP-IPC) ---
    // RCCL requires one distinct GPU per rank; when ranks share a device
    // (oversubscribed worlds, 1-GPU multi-worker nodes) the device data
    // plane falls back to PTP device messages — same-process staged D2D,
    // cross-process HIP-IPC arenas — with gfx950 elementwise kernels
    // doing the reductions. FAABRIC_DEVICE_PLANE=rccl|ptp overrides.
    bool rcclUsable(int rank);
    bool rcclBroken = false; // guarded by worldMx
    void devSend(int sendRank,
                 int recvRank,
                 const void* devPtr,
                 size_t bytes,
                 MpiMessageType type);
    void devRecv(int sendRank,
                 int recvRank,
                 void* devPtr,
                 size_t bytes,
                 MpiMessageType type);
    void* fbStream_ = nullptr; // lazily-created fallback stream
    void* fallbackStream();
    void deviceReduceFallback(int thisRank,
                              int rootRank,
                              const uint8_t* sendBuffer,
                              uint8_t* recvBuffer,
                              MpiDataType dataType,
                              int count,
                              MpiOp op);
    void deviceBroadcastFallback(int rootRank,
                                 int thisRank,
                                 uint8_t* buffer,
                                 size_t bytes,
                                 MpiMessageType type);

  public:
    // Host-plane combine inout[i] = op(inout[i], in[i]); stateless
    static void opReduceHost(MpiOp op,
                             MpiDataType type,
                             int count,
                             const uint8_t* in,
                             uint8_t* inout);
};

class MpiWorldRegistry
{
  public:
    static MpiWorldRegistry& get();
    MpiWorld& createWorld(Message& msg, int worldId);
    MpiWorld& getOrInitialiseWorld(Message& msg);
    MpiWorld& getWorld(int worldId);
    bool worldExists(int worldId);
    void clearWorld(int worldId);
    void clear();

  private:
    std::mutex mx;
    std::map<int, std::shared_ptr<MpiWorld>> worlds;
};

// Thread-local rank context (reference: mpi/MpiContext.h:7-27)
class MpiContext
{
  public:
    MpiContext();
    int createWorld(Message& msg);
    void joinWorld(Message& msg);
    bool getIsMpi() const { return isMpi; }
    int getRank() const { return rank; }
    int getWorldId() const { return worldId; }
    MpiWorld& getWorld();

  private:
    bool isMpi = false;
    int rank = -1;
    int worldId = -1;
};

MpiContext& getMpiContext(); // thread-local

} // namespace faabricamd

// Per-host scheduler: executor pool + function-call RPC + reaper
// (reference: include/faabric/scheduler/Scheduler.h:41,
//  src/scheduler/Scheduler.cpp:48-448,
//  src/scheduler/FunctionCallServer.cpp:21-95).
#pragma once

#include <memory>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>
#include <vector>

#include "faabricamd/executor.h"
#include "faabricamd/messages.h"
#include "faabricamd/queue.h"
#include "faabricamd/transport.h"

namespace faabricamd {

// RPC call codes (reference: scheduler/FunctionCallApi.h:4-10)
enum class FunctionCalls : uint8_t
{
    ExecuteFunctions = 1,
    Flush = 2,
    SetMessageResult = 3,
    BatchDone = 4,
};

class Scheduler
{
  public:
    static Scheduler& get();

    // Execute a batch scheduled to this host
    // (reference: src/scheduler/Scheduler.cpp:250)
    void executeBatch(std::shared_ptr<BatchExecuteRequest> req);

    // Resources advertised to the planner
    HostResources getThisHostResources();
    void setThisHostResources(const HostResources& res);

    // Periodic reaping of idle warm executors
    // (reference: src/scheduler/Scheduler.cpp:166-241)
    int reapStaleExecutors();
    void startReaper();
    void stopReaper();

    // Migration check entry point called periodically by long-running apps
    // (reference: src/scheduler/Scheduler.cpp:448)
    std::shared_ptr<PendingMigration> checkForMigrationOpportunities(
      Message& msg,
      int32_t overwriteNewGroupId = 0);

    void flushLocally();
    void shutdown();
    void reset();

    // Test-mode recording (reference: src/scheduler/Scheduler.cpp:263-268)
    std::vector<Message> getRecordedMessages();
    void clearRecordedMessages();

    size_t getExecutorCount();
    // Idle-list entries over all warm pools (stale ones included)
    size_t debugIdleCount();

  private:
    Scheduler();

    struct WarmPool
    {
        // Every executor of one function, claimed or not
        std::vector<std::shared_ptr<Executor>> list;
        // The unclaimed ones: Executor::releaseClaim pushes, claims pop in
        // O(1). A hint only: Executor::tryClaim decides ownership, so a
        // stale entry is dropped and can never cause a double claim.
        // Shared with the executors, which may outlive the pool.
        std::shared_ptr<Executor::IdleExecutors> idle =
          std::make_shared<Executor::IdleExecutors>();
    };

    std::shared_ptr<Executor> claimExecutor(Message& msg);
    // One executor per message of a FUNCTIONS batch: execs[i] is claimed
    // for messages[i], or null with errors[i] set if creating it failed
    void claimExecutors(BatchExecuteRequest& req,
                        std::vector<std::shared_ptr<Executor>>& execs,
                        std::vector<std::string>& errors);
    // Caller holds schedMx unique
    std::shared_ptr<Executor> createExecutorLocked(WarmPool& pool,
                                                   Message& msg);

    // Claims take the lock SHARED (they only pop the pool's idle list,
    // which has its own short lock); executor creation and reaping take
    // it unique.
    std::shared_mutex schedMx;
    std::unordered_map<std::string, std::unique_ptr<WarmPool>> executors;
    HostResources overriddenResources;
    bool resourcesOverridden = false;

    std::vector<Message> recordedMessages;

    class ReaperThread;
    std::shared_ptr<ReaperThread> reaper;
};

// True when this process runs a FunctionCallServer (i.e. BATCH_DONE
// pushes from the planner can actually reach it)
bool functionCallServerRunning();

class FunctionCallServer : public MessageEndpointServer
{
  public:
    FunctionCallServer();
    ~FunctionCallServer() override;
    void doAsyncRecv(uint8_t code,
                     const std::string& body,
                     uint32_t seq) override;
    std::string doSyncRecv(uint8_t code, const std::string& body) override;
};

class FunctionCallClient : public MessageEndpointClient
{
  public:
    explicit FunctionCallClient(const std::string& host);
    void executeFunctions(const BatchExecuteRequest& req);
    void setMessageResult(const Message& msg);
    void sendFlush();
    void batchDone(int32_t appId);
};

std::shared_ptr<FunctionCallClient> getFunctionCallClient(
  const std::string& host);

// Local BATCH_DONE flag registry (planner pushes, PlannerClient::
// waitBatchDone sleeps). prepare() before registering with the planner
// so a push can never be missed; discard() cleans up after the wait.
std::shared_ptr<FlagWaiter> batchDoneWaiterPrepare(int32_t appId);
void batchDoneWaiterDiscard(int32_t appId);
void signalBatchDone(int32_t appId);
void clearFunctionCallClients();

// Mock-mode recording (reference: src/scheduler/FunctionCallClient.cpp:14-99)
std::vector<std::pair<std::string, BatchExecuteRequest>>
getBatchRequestsSentMock();
void clearMockedFunctionCalls();

} // namespace faabricamd

// Per-host scheduler (reference behavior: src/scheduler/Scheduler.cpp
// :250-337 executeBatch, :339-387 claimExecutor, :166-241 reaper,
// :448-530 migration check; src/scheduler/FunctionCallServer.cpp:21-95).
#include "faabricamd/scheduler.h"
#include "faabricamd/utilextras.h"

#include <atomic>
#include <thread>
#include <functional>
#include <condition_variable>
#include "faabricamd/planner.h"
#include "faabricamd/ptp.h"
#include "faabricamd/util.h"
#include "faabricamd/wire.h"

#include <hip/hip_runtime.h>

namespace faabricamd {

// Cached GPU count; probing HIP is cheap but not free
static int getNumGpus()
{
    static int n = []() {
        const auto& conf = getSystemConfig();
        if (conf.overrideGpuCount >= 0) {
            return conf.overrideGpuCount;
        }
        if (!conf.useGpu) {
            return 0;
        }
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) {
            return 0;
        }
        return count;
    }();
    return n;
}

class Scheduler::ReaperThread : public PeriodicBackgroundThread
{
  public:
    void doWork() override { Scheduler::get().reapStaleExecutors(); }
};

Scheduler::Scheduler() = default;

Scheduler& Scheduler::get()
{
    static Scheduler sched;
    return sched;
}

HostResources Scheduler::getThisHostResources()
{
    {
        std::unique_lock<std::shared_mutex> lock(schedMx);
        if (resourcesOverridden) {
            return overriddenResources;
        }
    }
    HostResources res;
    // On an MI355X node a slot is a GPU; CPU-only hosts fall back to cores
    int nGpus = getNumGpus();
    res.slots = nGpus > 0 ? nGpus : getUsableCores();
    res.usedSlots = 0;
    return res;
}

void Scheduler::setThisHostResources(const HostResources& res)
{
    std::unique_lock<std::shared_mutex> lock(schedMx);
    overriddenResources = res;
    resourcesOverridden = true;
}

void Scheduler::executeBatch(std::shared_ptr<BatchExecuteRequest> req)
{
    if (req->messages.empty()) {
        return;
    }
    PROF_START(sched_execute_batch)
    bool isThreads = req->type == BatchExecuteType::THREADS;

    if (isTestMode()) {
        std::unique_lock<std::shared_mutex> lock(schedMx);
        for (const auto& msg : req->messages) {
            recordedMessages.push_back(msg);
        }
    }

    if (isThreads) {
        // One executor runs all local threads of the app
        // (reference: src/scheduler/Scheduler.cpp:272-298)
        auto exec = claimExecutor(req->messages[0]);
        std::vector<int> idxs(req->messages.size());
        for (size_t i = 0; i < idxs.size(); i++) {
            idxs[i] = (int)i;
        }
        exec->executeTasks(idxs, req);
    } else {
        // One executor per message, all claimed in one go: the warm ones
        // come off the pool's idle list in a single acquisition and the
        // pool grows once for the shortfall
        size_t n = req->messages.size();
        std::vector<std::shared_ptr<Executor>> execs;
        std::vector<std::string> claimErrors;
        PROF_START(dispatch_claim)
        claimExecutors(*req, execs, claimErrors);
        PROF_END(dispatch_claim)

        // Hand the tasks over one after the other on this thread. A
        // hand-off is a mailbox post plus, for a sleeping pool thread, one
        // futex wake, and that pace is what keeps the batch fast: fanning
        // the wakes out over helper threads (as the slower queue hand-off
        // once needed) starts every executor thread at once, they pile up
        // on the few CPUs and on the locks every task takes, and the
        // batch takes longer (profiles/dispatch_path_ab.json, lane sweep:
        // 8 lanes ran at about half the rate of 1 lane at 128 messages
        // and at a fifth at 1024)
        PROF_START(dispatch_enqueue)
        for (size_t i = 0; i < n; i++) {
            try {
                if (!execs[i]) {
                    throw FaabricException(claimErrors[i]);
                }
                execs[i]->executeSingleTask((int)i, req);
            } catch (const std::exception& e) {
                // Failures set an error result instead of crashing the host
                // (reference: src/scheduler/Scheduler.cpp:304-322)
                FAM_ERROR("claiming executor failed: %s", e.what());
                if (execs[i]) {
                    execs[i]->releaseClaim();
                }
                auto msg = std::make_shared<Message>(req->messages[i]);
                msg->returnValue = 1;
                msg->executedHost = getSystemConfig().endpointHost;
                msg->outputData = std::string("executor claim failed: ") +
                                  e.what();
                getPlannerClient().setMessageResult(msg);
            }
        }
        PROF_END(dispatch_enqueue)
    }
    PROF_END(sched_execute_batch)
}

// Caller holds schedMx (shared is enough). Pops idle-list entries until
// one wins the claim CAS; a stale entry (claimed meanwhile, or reaped and
// left claimed for good) is simply dropped.
static std::shared_ptr<Executor> popIdleClaimed(
  Executor::IdleExecutors& idle)
{
    std::shared_ptr<Executor> e;
    while (idle.pop(e)) {
        if (e->tryClaim()) {
            return e;
        }
    }
    return nullptr;
}

std::shared_ptr<Executor> Scheduler::createExecutorLocked(WarmPool& pool,
                                                          Message& msg)
{
    auto exec = getExecutorFactory()->createExecutor(msg);
    exec->claim();
    exec->setIdleList(pool.idle);
    if (getNumGpus() > 0) {
        const auto& conf = getSystemConfig();
        // A worker pinned to one GPU (FAABRIC_GPU_DEVICE) keeps every
        // executor there; a multi-GPU single process spreads them
        exec->gpuDevice =
          conf.gpuDevicePinned
            ? conf.gpuDevice
            : (int)((pool.list.size()) % (size_t)getNumGpus());
    }
    pool.list.push_back(exec);
    return exec;
}

std::shared_ptr<Executor> Scheduler::claimExecutor(Message& msg)
{
    std::string key = msg.user + "/" + msg.function;

    // Fast path: warm reuse under the SHARED lock, O(1) off the idle list
    // (reference: src/scheduler/Scheduler.cpp:339-387)
    {
        std::shared_lock<std::shared_mutex> rlock(schedMx);
        auto it = executors.find(key);
        if (it != executors.end()) {
            if (auto e = popIdleClaimed(*it->second->idle)) {
                return e;
            }
        }
    }

    // Slow path: grow the pool under the unique lock (re-check first —
    // an executor may have been released meanwhile)
    std::unique_lock<std::shared_mutex> lock(schedMx);
    auto& poolPtr = executors[key];
    if (!poolPtr) {
        poolPtr = std::make_unique<WarmPool>();
    }
    if (auto e = popIdleClaimed(*poolPtr->idle)) {
        return e;
    }
    return createExecutorLocked(*poolPtr, msg);
}

void Scheduler::claimExecutors(
  BatchExecuteRequest& req,
  std::vector<std::shared_ptr<Executor>>& execs,
  std::vector<std::string>& errors)
{
    size_t n = req.messages.size();
    execs.assign(n, nullptr);
    errors.assign(n, std::string());

    // Pools are per function: a batch that mixes functions (not what the
    // batch factory builds) claims message by message
    const Message& first = req.messages[0];
    bool oneFunction = true;
    for (size_t i = 1; i < n && oneFunction; i++) {
        oneFunction = req.messages[i].function == first.function &&
                      req.messages[i].user == first.user;
    }
    if (!oneFunction) {
        for (size_t i = 0; i < n; i++) {
            try {
                execs[i] = claimExecutor(req.messages[i]);
            } catch (const std::exception& e) {
                errors[i] = e.what();
            }
        }
        return;
    }

    std::string key = first.user + "/" + first.function;
    std::vector<std::shared_ptr<Executor>> popped;
    popped.reserve(n);
    size_t got = 0;
    // Take up to (n - got) idle entries in one acquisition, keep those
    // that win the claim CAS; repeat only if stale entries were dropped
    auto takeIdle = [&](Executor::IdleExecutors& idle) {
        while (got < n) {
            popped.clear();
            if (idle.popMany(n - got, popped) == 0) {
                return;
            }
            for (auto& e : popped) {
                if (e->tryClaim()) {
                    execs[got++] = std::move(e);
                }
            }
        }
    };
    {
        std::shared_lock<std::shared_mutex> rlock(schedMx);
        auto it = executors.find(key);
        if (it != executors.end()) {
            takeIdle(*it->second->idle);
        }
    }
    if (got == n) {
        return;
    }

    // Shortfall: grow the pool once, under one unique acquisition
    std::unique_lock<std::shared_mutex> lock(schedMx);
    auto& poolPtr = executors[key];
    if (!poolPtr) {
        poolPtr = std::make_unique<WarmPool>();
    }
    takeIdle(*poolPtr->idle);
    poolPtr->list.reserve(poolPtr->list.size() + (n - got));
    for (; got < n; got++) {
        try {
            execs[got] = createExecutorLocked(*poolPtr, req.messages[got]);
        } catch (const std::exception& e) {
            errors[got] = e.what();
        }
    }
}

int Scheduler::reapStaleExecutors()
{
    std::unique_lock<std::shared_mutex> lock(schedMx);
    const auto& conf = getSystemConfig();
    int reaped = 0;
    for (auto& [key, pool] : executors) {
        auto& list = pool->list;
        for (auto it = list.begin(); it != list.end();) {
            auto& exec = *it;
            // Reaping takes the claim and never gives it back: an idle-list
            // entry pushed by a release that raced with this check then
            // loses its CAS and is dropped by whoever pops it
            if (exec->getMillisSinceLastExec() > conf.boundTimeout &&
                exec->tryClaim()) {
                pool->idle->remove(exec);
                exec->shutdown();
                it = list.erase(it);
                reaped++;
            } else {
                ++it;
            }
        }
    }
    return reaped;
}

void Scheduler::startReaper()
{
    if (!reaper) {
        reaper = std::make_shared<ReaperThread>();
        reaper->startMillis(getSystemConfig().boundTimeout);
    }
}

void Scheduler::stopReaper()
{
    if (reaper) {
        reaper->stop();
        reaper = nullptr;
    }
}

std::shared_ptr<PendingMigration> Scheduler::checkForMigrationOpportunities(
  Message& msg,
  int32_t overwriteNewGroupId)
{
    // Group idx 0 asks the planner (DIST_CHANGE); the rest of the group
    // receive the verdict over a dedicated PTP channel
    // (reference: src/scheduler/Scheduler.cpp:448-530)
    int32_t newGroupId = 0;
    if (msg.groupIdx == 0 && overwriteNewGroupId == 0) {
        auto req = std::make_shared<BatchExecuteRequest>();
        req->appId = msg.appId;
        req->groupId = msg.groupId;
        req->user = msg.user;
        req->function = msg.function;
        req->type = BatchExecuteType::MIGRATION;
        auto decision = getPlannerClient().callFunctions(req);
        if (decision->appId == DO_NOT_MIGRATE) {
            newGroupId = 0;
        } else if (decision->appId == MUST_FREEZE) {
            newGroupId = MUST_FREEZE;
        } else {
            newGroupId = decision->groupId;
        }
        // Tell the rest of the group
        auto& broker = getPointToPointBroker();
        int32_t payload = newGroupId;
        for (int i = 1; i < msg.groupSize; i++) {
            broker.sendMessage(msg.appId,
                               msg.groupId,
                               PTP_MIGRATION_CHANNEL_OFFSET,
                               i,
                               (const uint8_t*)&payload,
                               sizeof(payload));
        }
    } else if (overwriteNewGroupId != 0) {
        newGroupId = overwriteNewGroupId;
    } else {
        auto data = getPointToPointBroker().recvMessage(
          msg.groupId, PTP_MIGRATION_CHANNEL_OFFSET, msg.groupIdx);
        newGroupId = *(const int32_t*)data.data();
    }

    if (newGroupId == 0) {
        return nullptr;
    }

    auto migration = std::make_shared<PendingMigration>();
    migration->appId = msg.appId;
    migration->groupIdx = msg.groupIdx;
    migration->srcHost = getSystemConfig().endpointHost;

    if (newGroupId == MUST_FREEZE) {
        migration->appId = MUST_FREEZE;
        return migration;
    }

    // A migration is happening: find out where THIS message now lives
    migration->groupId = newGroupId;
    auto decision = getPlannerClient().getSchedulingDecision(msg.appId);
    for (int i = 0; i < decision.nFunctions; i++) {
        if (decision.groupIdxs[i] == msg.groupIdx) {
            migration->dstHost = decision.hosts[i];
            break;
        }
    }
    return migration;
}

void Scheduler::flushLocally()
{
    std::unique_lock<std::shared_mutex> lock(schedMx);
    for (auto& [key, pool] : executors) {
        pool->idle->close();
        for (auto& e : pool->list) {
            e->flush();
        }
    }
    executors.clear();
    getExecutorFactory()->flushHost();
}

void Scheduler::shutdown()
{
    stopReaper();
    std::unique_lock<std::shared_mutex> lock(schedMx);
    for (auto& [key, pool] : executors) {
        pool->idle->close();
        for (auto& e : pool->list) {
            e->shutdown();
        }
    }
    executors.clear();
}

void Scheduler::reset()
{
    shutdown();
    std::unique_lock<std::shared_mutex> lock(schedMx);
    recordedMessages.clear();
    resourcesOverridden = false;
}

std::vector<Message> Scheduler::getRecordedMessages()
{
    std::unique_lock<std::shared_mutex> lock(schedMx);
    return recordedMessages;
}

void Scheduler::clearRecordedMessages()
{
    std::unique_lock<std::shared_mutex> lock(schedMx);
    recordedMessages.clear();
}

size_t Scheduler::getExecutorCount()
{
    std::unique_lock<std::shared_mutex> lock(schedMx);
    size_t n = 0;
    for (auto& [key, pool] : executors) {
        n += pool->list.size();
    }
    return n;
}

size_t Scheduler::debugIdleCount()
{
    std::shared_lock<std::shared_mutex> lock(schedMx);
    size_t n = 0;
    for (auto& [key, pool] : executors) {
        n += pool->idle->size();
    }
    return n;
}

// ------------------------- RPC server / client ------------------------------

static std::atomic<int> fnServersUp{ 0 };

bool functionCallServerRunning()
{
    return fnServersUp.load(std::memory_order_relaxed) > 0;
}

FunctionCallServer::FunctionCallServer()
  : MessageEndpointServer(FUNCTION_CALL_ASYNC_PORT,
                          FUNCTION_CALL_SYNC_PORT,
                          "function-call")
{
    fnServersUp.fetch_add(1, std::memory_order_relaxed);
}

FunctionCallServer::~FunctionCallServer()
{
    fnServersUp.fetch_sub(1, std::memory_order_relaxed);
}

// ------------------- local BATCH_DONE flag registry -------------------------

static std::mutex batchDoneMx;
static std::map<int32_t, std::shared_ptr<FlagWaiter>> batchDoneFlags;

std::shared_ptr<FlagWaiter> batchDoneWaiterPrepare(int32_t appId)
{
    std::lock_guard<std::mutex> lock(batchDoneMx);
    auto& w = batchDoneFlags[appId];
    if (!w) {
        w = std::make_shared<FlagWaiter>();
    }
    return w;
}

void batchDoneWaiterDiscard(int32_t appId)
{
    std::lock_guard<std::mutex> lock(batchDoneMx);
    batchDoneFlags.erase(appId);
}

void signalBatchDone(int32_t appId)
{
    std::shared_ptr<FlagWaiter> w;
    {
        std::lock_guard<std::mutex> lock(batchDoneMx);
        auto it = batchDoneFlags.find(appId);
        if (it == batchDoneFlags.end()) {
            return; // push for a wait that already gave up
        }
        w = it->second;
    }
    w->setFlag(true);
}

void FunctionCallServer::doAsyncRecv(uint8_t code,
                                     const std::string& body,
                                     uint32_t seq)
{
    (void)seq;
    switch ((FunctionCalls)code) {
        case FunctionCalls::ExecuteFunctions: {
            PROF_START(exec_decode)
            auto req = std::make_shared<BatchExecuteRequest>(
              BatchExecuteRequest::decode(body));
            PROF_END(exec_decode)
            Scheduler::get().executeBatch(req);
            break;
        }
        case FunctionCalls::SetMessageResult: {
            auto msg = std::make_shared<Message>(Message::decode(body));
            getPlannerClient().setMessageResultLocally(msg);
            break;
        }
        case FunctionCalls::BatchDone: {
            PbReader r(body);
            int32_t appId = 0;
            uint32_t f;
            WireType t;
            while (r.next(f, t)) {
                if (f == 1) {
                    appId = (int32_t)r.varint();
                } else {
                    r.skip(t);
                }
            }
            signalBatchDone(appId);
            break;
        }
        default:
            FAM_ERROR("function call server: bad async code %d", (int)code);
    }
}

std::string FunctionCallServer::doSyncRecv(uint8_t code,
                                           const std::string& body)
{
    (void)body;
    if ((FunctionCalls)code == FunctionCalls::Flush) {
        Scheduler::get().flushLocally();
        return {};
    }
    throw FaabricException("function call server: bad sync code " +
                           std::to_string(code));
}

FunctionCallClient::FunctionCallClient(const std::string& host)
  : MessageEndpointClient(host,
                          FUNCTION_CALL_ASYNC_PORT,
                          FUNCTION_CALL_SYNC_PORT)
{}

// Mock-mode recording
static std::mutex mockMx;
static std::vector<std::pair<std::string, BatchExecuteRequest>>
  mockedBatchRequests;

std::vector<std::pair<std::string, BatchExecuteRequest>>
getBatchRequestsSentMock()
{
    std::lock_guard<std::mutex> lock(mockMx);
    return mockedBatchRequests;
}

void clearMockedFunctionCalls()
{
    std::lock_guard<std::mutex> lock(mockMx);
    mockedBatchRequests.clear();
}

void FunctionCallClient::executeFunctions(const BatchExecuteRequest& req)
{
    if (isMockMode()) {
        std::lock_guard<std::mutex> lock(mockMx);
        mockedBatchRequests.emplace_back(getHost(), req);
        return;
    }
    asyncSend((uint8_t)FunctionCalls::ExecuteFunctions, req.encode());
}

void FunctionCallClient::setMessageResult(const Message& msg)
{
    if (isMockMode()) {
        return;
    }
    asyncSend((uint8_t)FunctionCalls::SetMessageResult, msg.encode());
}

void FunctionCallClient::batchDone(int32_t appId)
{
    if (isMockMode()) {
        return;
    }
    PbWriter w;
    w.putInt32(1, appId);
    std::string body = w.take();
    asyncSend((uint8_t)FunctionCalls::BatchDone, body.data(), body.size());
}

void FunctionCallClient::sendFlush()
{
    syncSend((uint8_t)FunctionCalls::Flush, "");
}

static std::mutex fcClientsMx;
static std::map<std::string, std::shared_ptr<FunctionCallClient>> fcClients;

std::shared_ptr<FunctionCallClient> getFunctionCallClient(
  const std::string& host)
{
    std::lock_guard<std::mutex> lock(fcClientsMx);
    auto& cli = fcClients[host];
    if (!cli) {
        cli = std::make_shared<FunctionCallClient>(host);
    }
    return cli;
}

void clearFunctionCallClients()
{
    std::lock_guard<std::mutex> lock(fcClientsMx);
    fcClients.clear();
}

} // namespace faabricamd

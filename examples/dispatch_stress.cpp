// Stand-alone stress of the dispatch hand-off primitives (Mailbox and
// IdleList from faabricamd/mailbox.h). Host C++ only: no HIP, no Python,
// no other project code, so it builds under -fsanitize=thread and
// -fsanitize=address,undefined (make stress-tsan / stress-asan).
//
// Model: EXECUTORS fake executors, each with a claim flag, one mailbox and
// one consumer thread, all sharing one idle list, exactly like a warm
// pool. LANES producer threads claim batches of executors off the idle
// list (pop, then the claim CAS), post one numbered task to each and move
// on; a consumer runs the task and releases its executor (unclaim, then
// push). A "thief" thread claims executors by scanning past the idle
// list, which plants stale and duplicate entries the way a racing release
// does. Checks: every task is delivered exactly once, in-use flags never
// overlap (no double claim), multi-task bursts arrive in order, and a
// timed take() on an empty mailbox returns false.
#include "faabricamd/mailbox.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <vector>

using faabricamd::IdleList;
using faabricamd::Mailbox;

namespace {

struct Task
{
    int64_t id = -1; // -1: stop
    int burstSeq = 0;
};

struct FakeExecutor
{
    std::atomic<bool> claimed{ false };
    std::atomic<int> inUse{ 0 };
    Mailbox<Task> mailbox;
    std::thread thread;
    int lastBurstSeq = -1;

    bool tryClaim()
    {
        bool expected = false;
        return claimed.compare_exchange_strong(expected, true);
    }
};

constexpr int EXECUTORS = 48;
constexpr int LANES = 6;
constexpr int BATCH = 12;

std::atomic<int> failures{ 0 };

void fail(const char* what)
{
    std::fprintf(stderr, "FAIL: %s\n", what);
    failures.fetch_add(1);
}

} // namespace

int main(int argc, char** argv)
{
    double seconds = argc > 1 ? std::atof(argv[1]) : 1.5;

    // --- timed take on an empty mailbox -----------------------------------
    {
        Mailbox<Task> empty;
        Task t;
        auto t0 = std::chrono::steady_clock::now();
        if (empty.take(t, 30)) {
            fail("take() on an empty mailbox returned a task");
        }
        auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                    std::chrono::steady_clock::now() - t0)
                    .count();
        if (ms < 25 || ms > 2000) {
            fail("timed take() did not honour its timeout");
        }
    }

    // --- ordered bursts beyond the slot count ------------------------------
    {
        Mailbox<Task, 4> small;
        constexpr int N = 200;
        std::thread consumer([&] {
            for (int i = 0; i < N; i++) {
                Task t;
                while (!small.take(t, 50)) {
                }
                if (t.burstSeq != i) {
                    fail("burst arrived out of order");
                }
            }
        });
        for (int i = 0; i < N; i++) {
            Task t;
            t.id = i;
            t.burstSeq = i;
            small.post(t);
        }
        consumer.join();
    }

    // --- pool model --------------------------------------------------------
    std::vector<std::unique_ptr<FakeExecutor>> execs;
    auto idle = std::make_shared<IdleList<FakeExecutor*>>();
    constexpr int64_t MAX_TASKS = 1 << 22;
    std::unique_ptr<std::atomic<uint8_t>[]> delivered(
      new std::atomic<uint8_t>[MAX_TASKS]);
    for (int64_t i = 0; i < MAX_TASKS; i++) {
        delivered[i].store(0, std::memory_order_relaxed);
    }
    std::atomic<int64_t> nextTaskId{ 0 };
    std::atomic<int64_t> completed{ 0 };

    for (int i = 0; i < EXECUTORS; i++) {
        execs.push_back(std::make_unique<FakeExecutor>());
    }
    for (auto& ePtr : execs) {
        FakeExecutor* e = ePtr.get();
        e->thread = std::thread([e, idle, &delivered, &completed] {
            while (true) {
                Task t;
                if (!e->mailbox.take(t, 20)) {
                    continue; // bound-timeout wake-up: nothing to do
                }
                if (t.id < 0) {
                    return;
                }
                if (e->inUse.fetch_add(1) != 0) {
                    fail("executor ran two tasks at once");
                }
                if (!e->claimed.load()) {
                    fail("task ran on an unclaimed executor");
                }
                if (delivered[t.id].fetch_add(1) != 0) {
                    fail("task delivered twice");
                }
                e->inUse.fetch_sub(1);
                completed.fetch_add(1);
                // releaseClaim(): unclaim, then advertise
                e->claimed.store(false);
                idle->push(e);
            }
        });
        idle->push(e);
    }

    std::atomic<bool> stop{ false };
    std::vector<std::thread> lanes;
    for (int l = 0; l < LANES; l++) {
        lanes.emplace_back([&] {
            std::vector<FakeExecutor*> popped;
            while (!stop.load()) {
                popped.clear();
                idle->popMany(BATCH, popped);
                for (FakeExecutor* e : popped) {
                    if (!e->tryClaim()) {
                        continue; // stale or duplicate entry: drop it
                    }
                    int64_t id = nextTaskId.fetch_add(1);
                    if (id >= MAX_TASKS) {
                        e->claimed.store(false);
                        idle->push(e);
                        stop.store(true);
                        break;
                    }
                    Task t;
                    t.id = id;
                    e->mailbox.post(t);
                }
                if (popped.empty()) {
                    std::this_thread::yield();
                }
            }
        });
    }
    // The thief claims without popping, so the later release of that
    // executor leaves a second entry behind the one still on the list
    std::thread thief([&] {
        size_t i = 0;
        while (!stop.load()) {
            FakeExecutor* e = execs[i++ % execs.size()].get();
            if (e->tryClaim()) {
                int64_t id = nextTaskId.fetch_add(1);
                if (id >= MAX_TASKS) {
                    e->claimed.store(false);
                    stop.store(true);
                    break;
                }
                Task t;
                t.id = id;
                e->mailbox.post(t);
            }
            std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
    });
    // remove() while everything runs (the reaper's path): a removed
    // executor is simply pushed back
    std::thread remover([&] {
        size_t i = 0;
        while (!stop.load()) {
            FakeExecutor* e = execs[i++ % execs.size()].get();
            if (e->tryClaim()) {
                idle->remove(e);
                e->claimed.store(false);
                idle->push(e);
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    });

    std::this_thread::sleep_for(
      std::chrono::milliseconds((int)(seconds * 1000)));
    stop.store(true);
    for (auto& t : lanes) {
        t.join();
    }
    thief.join();
    remover.join();

    // Drain: every posted task completes, then stop the consumers
    int64_t posted = std::min<int64_t>(nextTaskId.load(), MAX_TASKS);
    auto deadline =
      std::chrono::steady_clock::now() + std::chrono::seconds(30);
    while (completed.load() < posted &&
           std::chrono::steady_clock::now() < deadline) {
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    for (auto& e : execs) {
        Task stopTask;
        e->mailbox.post(stopTask);
    }
    for (auto& e : execs) {
        e->thread.join();
    }
    idle->close();

    if (completed.load() != posted) {
        fail("not every posted task completed");
    }
    for (int64_t i = 0; i < posted; i++) {
        if (delivered[i].load(std::memory_order_relaxed) != 1) {
            fail("a task was not delivered exactly once");
            break;
        }
    }
    if (posted < 1000) {
        fail("stress made no progress");
    }

    std::printf("dispatch_stress: %lld tasks over %d executors, %d lanes: %s\n",
                (long long)posted,
                EXECUTORS,
                LANES,
                failures.load() == 0 ? "OK" : "FAILED");
    return failures.load() == 0 ? 0 : 1;
}

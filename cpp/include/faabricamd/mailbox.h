// Hand-off primitives of the batch dispatch path. Header-only and free of
// any other project header, so examples/dispatch_stress.cpp can exercise
// them on their own under the thread and address sanitizers.
//
//  - Mailbox<T>:  small bounded many-producer/one-consumer ring an executor
//                 pool thread sleeps on. Posting is one ticket fetch_add and
//                 one slot store, plus one futex wake only when the consumer
//                 sleeps; no mutex is shared between the two sides.
//  - IdleList<T>: LIFO of unclaimed executors of one warm pool. A hint
//                 only: ownership stays with the executor's claim CAS, so a
//                 stale or duplicate entry can never cause a double claim.
#pragma once

#include <atomic>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <ctime>
#include <mutex>
#include <utility>
#include <vector>

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

namespace faabricamd {

namespace detail {

// Sleep while *word == expected, at most timeoutMs (<= 0: no limit).
// Spurious returns are fine: callers re-check their condition.
inline void futexWait(std::atomic<uint32_t>* word,
                      uint32_t expected,
                      int timeoutMs)
{
    static_assert(sizeof(std::atomic<uint32_t>) == sizeof(uint32_t));
    struct timespec ts;
    struct timespec* tsp = nullptr;
    if (timeoutMs > 0) {
        ts.tv_sec = timeoutMs / 1000;
        ts.tv_nsec = (long)(timeoutMs % 1000) * 1000000L;
        tsp = &ts;
    }
    syscall(SYS_futex,
            reinterpret_cast<uint32_t*>(word),
            FUTEX_WAIT_PRIVATE,
            expected,
            tsp,
            nullptr,
            0);
}

inline void futexWake(std::atomic<uint32_t>* word, int n)
{
    syscall(SYS_futex,
            reinterpret_cast<uint32_t*>(word),
            FUTEX_WAKE_PRIVATE,
            n,
            nullptr,
            nullptr,
            0);
}

} // namespace detail

template<typename T, uint32_t SLOTS = 8>
class Mailbox
{
    static_assert(SLOTS >= 2 && (SLOTS & (SLOTS - 1)) == 0,
                  "SLOTS must be a power of two");

  public:
    Mailbox()
    {
        for (uint32_t i = 0; i < SLOTS; i++) {
            slots[i].seq.store(i, std::memory_order_relaxed);
        }
    }
    Mailbox(const Mailbox&) = delete;
    Mailbox& operator=(const Mailbox&) = delete;

    // Any thread. Blocks only while all SLOTS are occupied (more tasks
    // queued on one pool thread than the ring holds): that rare case
    // re-checks every millisecond until the consumer frees the slot.
    void post(T value)
    {
        uint32_t ticket = tail.fetch_add(1, std::memory_order_relaxed);
        Slot& s = slots[ticket & (SLOTS - 1)];
        uint32_t seen;
        while ((seen = s.seq.load(std::memory_order_acquire)) != ticket) {
            detail::futexWait(&s.seq, seen, 1);
        }
        s.value = std::move(value);
        // seq_cst store, then seq_cst load of `sleeping`: pairs with the
        // consumer's store of `sleeping` followed by its re-check of seq,
        // so one side always sees the other (no lost wake-up)
        s.seq.store(ticket + 1, std::memory_order_seq_cst);
        if (sleeping.load(std::memory_order_seq_cst) != 0) {
            detail::futexWake(&s.seq, INT_MAX);
        }
    }

    // The one consumer thread. False when nothing arrived within
    // timeoutMs (<= 0 waits without limit).
    bool take(T& out, int timeoutMs)
    {
        Slot& s = slots[head & (SLOTS - 1)];
        uint32_t ready = head + 1;
        uint32_t seen = s.seq.load(std::memory_order_acquire);
        if (seen != ready) {
            struct timespec start;
            clock_gettime(CLOCK_MONOTONIC, &start);
            int leftMs = timeoutMs;
            while (true) {
                sleeping.store(1, std::memory_order_seq_cst);
                seen = s.seq.load(std::memory_order_seq_cst);
                if (seen != ready) {
                    detail::futexWait(&s.seq, seen, leftMs);
                    seen = s.seq.load(std::memory_order_acquire);
                }
                sleeping.store(0, std::memory_order_relaxed);
                if (seen == ready) {
                    break;
                }
                if (timeoutMs > 0) {
                    struct timespec now;
                    clock_gettime(CLOCK_MONOTONIC, &now);
                    int64_t goneMs =
                      (int64_t)(now.tv_sec - start.tv_sec) * 1000 +
                      (now.tv_nsec - start.tv_nsec) / 1000000;
                    if (goneMs >= timeoutMs) {
                        return false;
                    }
                    leftMs = (int)(timeoutMs - goneMs);
                }
            }
        }
        out = std::move(s.value);
        s.value = T();
        // Hand the slot to the producer holding ticket head + SLOTS; one
        // that already polls for it sees the new value within its 1 ms
        s.seq.store(head + SLOTS, std::memory_order_release);
        head++;
        return true;
    }

  private:
    struct alignas(64) Slot
    {
        std::atomic<uint32_t> seq{ 0 };
        T value{};
    };
    Slot slots[SLOTS];
    alignas(64) std::atomic<uint32_t> tail{ 0 };
    std::atomic<uint32_t> sleeping{ 0 };
    // Consumer-private
    alignas(64) uint32_t head = 0;
};

template<typename T>
class IdleList
{
  public:
    // Ignored once closed (an executor finishing after a flush)
    void push(T value)
    {
        std::lock_guard<std::mutex> lock(mx);
        if (!closed) {
            entries.push_back(std::move(value));
        }
    }

    // Moves up to n entries to the back of `out` in ONE lock acquisition,
    // most recently released first; returns how many
    size_t popMany(size_t n, std::vector<T>& out)
    {
        std::lock_guard<std::mutex> lock(mx);
        size_t got = 0;
        while (got < n && !entries.empty()) {
            out.push_back(std::move(entries.back()));
            entries.pop_back();
            got++;
        }
        return got;
    }

    bool pop(T& out)
    {
        std::lock_guard<std::mutex> lock(mx);
        if (entries.empty()) {
            return false;
        }
        out = std::move(entries.back());
        entries.pop_back();
        return true;
    }

    // Drops every entry equal to `value` (the reaper's exit door)
    size_t remove(const T& value)
    {
        std::lock_guard<std::mutex> lock(mx);
        size_t before = entries.size();
        size_t w = 0;
        for (size_t r = 0; r < entries.size(); r++) {
            if (!(entries[r] == value)) {
                if (w != r) {
                    entries[w] = std::move(entries[r]);
                }
                w++;
            }
        }
        entries.resize(w);
        return before - w;
    }

    // Drops everything and refuses later pushes
    void close()
    {
        std::vector<T> dropped;
        {
            std::lock_guard<std::mutex> lock(mx);
            closed = true;
            dropped.swap(entries);
        }
    }

    size_t size()
    {
        std::lock_guard<std::mutex> lock(mx);
        return entries.size();
    }

  private:
    std::mutex mx;
    std::vector<T> entries;
    bool closed = false;
};

} // namespace faabricamd

// Util parity extras: page-delta codec, PROF timers, crash handler, CPU
// pinning (reference: src/util/delta.cpp, util/timing.h:6-17,
// src/util/crash.cpp:15-67, util/hwloc.h:31).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace faabricamd {

// ------------------------- delta codec --------------------------------------
// Page-wise XOR-against-old + zstd compression, config string
// "pages=4096;xor;zstd=1" like the reference (src/util/config.cpp:27,
// delta.cpp:15-57); "zlib=1" selects a zlib fallback. Stream format is
// command-tagged like the reference's (delta.cpp:155-169).

struct DeltaConfig
{
    size_t pageSize = 4096;
    bool xorWithOld = true;
    bool compress = true;
    // zstd by default, matching the reference's "pages=4096;xor;zstd=1"
    // (src/util/config.cpp:27); "zlib=1" selects the zlib fallback
    bool useZstd = true;

    static DeltaConfig parse(const std::string& s);
    std::string str() const;
};

// Encode new against old (old may be shorter; the tail ships raw)
std::vector<uint8_t> deltaEncode(const std::vector<uint8_t>& oldData,
                                 const std::vector<uint8_t>& newData,
                                 const DeltaConfig& conf = {});

// Apply a delta to old, producing new
std::vector<uint8_t> deltaApply(const std::vector<uint8_t>& oldData,
                                const std::vector<uint8_t>& delta);

// ------------------------- PROF timers --------------------------------------
// Compile-time-free runtime timers: totals aggregated per name
// (reference: util/timing.h PROF_START/PROF_END under TRACE_ALL)

void profStart(const std::string& name);
void profEnd(const std::string& name);
// True when FAABRIC_PROF=1; every timer below is a no-op otherwise
bool profEnabled();
// Steady-clock nanoseconds, for scopes that start and end on different
// threads (profStart/profEnd pair up per thread)
int64_t profNowNs();
// Add one measured duration to the totals of `name`
void profRecord(const char* name, double ms);
std::vector<std::pair<std::string, double>> profTotalsMs();
void profClear();
std::string profSummary();

// The enabled check comes first so a disabled timer builds no std::string
#define PROF_START(name)                                                       \
    if (::faabricamd::profEnabled()) {                                         \
        ::faabricamd::profStart(#name);                                        \
    }
#define PROF_END(name)                                                         \
    if (::faabricamd::profEnabled()) {                                         \
        ::faabricamd::profEnd(#name);                                          \
    }

// Scope timer for functions with several return paths
class ProfScope
{
  public:
    explicit ProfScope(const char* nameIn)
      : name(nameIn)
      , startNs(profEnabled() ? profNowNs() : 0)
    {}
    ~ProfScope()
    {
        if (startNs != 0) {
            profRecord(name, (double)(profNowNs() - startNs) / 1e6);
        }
    }
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;

  private:
    const char* name;
    int64_t startNs;
};

// ------------------------- crash handler ------------------------------------
// Backtrace-printing handlers for SIGABRT/SIGILL/SIGFPE; SIGSEGV stays
// free for the segfault dirty tracker (reference: src/util/crash.cpp:40-67)
void setUpCrashHandler();

// ------------------------- CPU pinning --------------------------------------
// Pin the calling thread to a free core from the process-wide pool;
// returns the core id or -1 (reference: util/hwloc.h pinThreadToFreeCpu)
int pinThreadToFreeCpu();
void unpinThisThread();

} // namespace faabricamd

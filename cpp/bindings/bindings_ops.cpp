// Ops bindings: the gfx950 snapshot engine (dirty pages, XOR diff, merge)
// and elementwise device reductions, plus the BASELINE config-4 benchmark
// loop (4 GB diff+merge) implemented natively.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "faabricamd/executor.h"
#include "faabricamd/ops.h"
#include "faabricamd/util.h"

#include <random>

namespace py = pybind11;
using namespace faabricamd;

namespace {

struct SnapBenchResult
{
    size_t bytes = 0;
    size_t nPages = 0;
    uint32_t dirtyPages = 0;
    double diffMean = 0;
    double applyMean = 0;
    std::vector<double> diffMs;
    std::vector<double> applyMs;
};

// Config-4 benchmark: region of `bytes` with `dirtyPct`% of pages dirty;
// each iteration runs the full diff (compare+compact) + merge (apply)
// pipeline on-device.
SnapBenchResult benchSnapshotPipelineImpl(size_t bytes,
                                          int iters,
                                          int warmup,
                                          double dirtyPct,
                                          int device)
{
    if (!gpuAvailable()) {
        throw FaabricException("snapshot pipeline bench needs a GPU");
    }
    if (hipSetDevice(device) != hipSuccess) {
        throw FaabricException("hipSetDevice failed");
    }

    size_t nPages = bytes / DEVICE_PAGE;
    DeviceSnapshot snap(bytes, device);

    // Updated view U: whole-region pseudo-random bytes (device-side
    // fill; every 8-byte word unique — no tiling the cache could love)
    uint8_t* updated = nullptr;
    if (hipMalloc(&updated, bytes) != hipSuccess) {
        throw FaabricException("hipMalloc updated failed");
    }
    famFillRandom(updated, bytes, 42, nullptr);
    hipDeviceSynchronize();
    snap.captureFromDevice(updated);

    // Dirty a RANDOMLY SCATTERED subset of pages in U by XOR-flipping
    // them (BASELINE config 4 asks for randomized dirty distribution,
    // not a stride or contiguous run)
    uint32_t nDirtyTarget = (uint32_t)((double)nPages * dirtyPct / 100.0);
    if (nDirtyTarget == 0 && dirtyPct > 0) {
        nDirtyTarget = 1;
    }
    if (nDirtyTarget > 0) {
        std::vector<uint32_t> all(nPages);
        for (uint32_t i = 0; i < nPages; i++) {
            all[i] = i;
        }
        std::mt19937_64 gen(1234);
        std::shuffle(all.begin(), all.end(), gen);
        std::vector<uint32_t> pages(all.begin(),
                                    all.begin() + nDirtyTarget);
        uint32_t* pagesDev = nullptr;
        uint8_t* flipDev = nullptr;
        hipMalloc(&pagesDev, nDirtyTarget * sizeof(uint32_t));
        // famApplyXorPages reads the payload SPARSELY (indexed by page),
        // so the flip buffer must span the whole region
        if (hipMalloc(&flipDev, bytes) != hipSuccess) {
            hipFree(pagesDev);
            hipFree(updated);
            throw FaabricException("hipMalloc flip buffer failed");
        }
        hipMemcpy(pagesDev,
                  pages.data(),
                  nDirtyTarget * sizeof(uint32_t),
                  hipMemcpyHostToDevice);
        hipMemset(flipDev, 0x5a, bytes);
        famApplyXorPages(updated, pagesDev, flipDev, nDirtyTarget, nullptr);
        hipDeviceSynchronize();
        hipFree(pagesDev);
        hipFree(flipDev);
    }

    std::vector<double> diffMs;
    std::vector<double> applyMs;
    uint32_t nd = 0;
    for (int it = 0; it < warmup + iters; it++) {
        int64_t t0 = getEpochMicros();
        nd = snap.diffXor(updated);
        int64_t t1 = getEpochMicros();
        snap.applyLastDiff();
        int64_t t2 = getEpochMicros();
        if (it >= warmup) {
            diffMs.push_back((t1 - t0) / 1000.0);
            applyMs.push_back((t2 - t1) / 1000.0);
        }
        // After the merge the snapshot equals U on the dirty pages, so
        // re-flip U's dirty set by XORing the (still resident) payload
        // back into U — keeps every iteration's dirty count identical.
        if (nd > 0) {
            famApplyXorPages(updated,
                             snap.diffPageIdx(),
                             snap.diffPayload(),
                             nd,
                             snap.stream());
            hipStreamSynchronize(snap.stream());
        }
    }
    hipFree(updated);

    SnapBenchResult res;
    res.bytes = bytes;
    res.nPages = nPages;
    res.dirtyPages = nd;
    for (double v : diffMs) {
        res.diffMean += v;
    }
    for (double v : applyMs) {
        res.applyMean += v;
    }
    res.diffMean /= std::max<size_t>(1, diffMs.size());
    res.applyMean /= std::max<size_t>(1, applyMs.size());
    res.diffMs = std::move(diffMs);
    res.applyMs = std::move(applyMs);
    return res;
}

py::dict benchSnapshotPipeline(size_t bytes,
                               int iters,
                               int warmup,
                               double dirtyPct,
                               int device)
{
    SnapBenchResult r;
    {
        py::gil_scoped_release release;
        r = benchSnapshotPipelineImpl(bytes, iters, warmup, dirtyPct,
                                      device);
    }
    // Diff reads both buffers fully + writes the payload; apply reads
    // payload+indices and read-modify-writes the dirty pages
    double dirtyBytes = (double)r.dirtyPages * DEVICE_PAGE;
    double diffBytes = 2.0 * (double)r.bytes + dirtyBytes;
    double applyBytes = 3.0 * dirtyBytes;

    py::dict out;
    out["bytes"] = r.bytes;
    out["n_pages"] = r.nPages;
    out["dirty_pages"] = r.dirtyPages;
    out["diff_ms"] = r.diffMean;
    out["apply_ms"] = r.applyMean;
    out["diff_gbps"] =
      r.diffMean > 0 ? diffBytes / (r.diffMean / 1e3) / 1e9 : 0;
    out["apply_gbps"] =
      r.applyMean > 0 ? applyBytes / (r.applyMean / 1e3) / 1e9 : 0;
    out["pipeline_gbps"] =
      (r.diffMean + r.applyMean) > 0
        ? (diffBytes + applyBytes) /
            ((r.diffMean + r.applyMean) / 1e3) / 1e9
        : 0;
    out["diff_ms_all"] = r.diffMs;
    out["apply_ms_all"] = r.applyMs;
    return out;
}

} // namespace

void initOpsBindings(py::module_& m)
{
    m.def("gpu_available", &gpuAvailable);
    m.def("gpu_count", &gpuCount);
    m.def("device_snapshot_exists", [](const std::string& key) {
        return DeviceSnapshotRegistry::get().snapshotExists(key);
    });
    m.def("device_snapshot_read",
          [](const std::string& key, size_t offset, size_t len) {
              auto snap = DeviceSnapshotRegistry::get().getSnapshot(key);
              std::vector<uint8_t> out(len);
              {
                  py::gil_scoped_release release;
                  snap->copyOutHost(out.data(), len, offset);
              }
              return py::bytes((const char*)out.data(), out.size());
          },
          py::arg("key"),
          py::arg("offset"),
          py::arg("len"));

    py::class_<DeviceSnapshot>(m, "DeviceSnapshot")
      .def(py::init<size_t, int>(), py::arg("bytes"), py::arg("device") = 0)
      .def_property_readonly("size", &DeviceSnapshot::size)
      .def_property_readonly("device", &DeviceSnapshot::device)
      .def_property_readonly("data_ptr",
                             [](DeviceSnapshot& s) {
                                 return (uintptr_t)s.data();
                             })
      .def("copy_in_host",
           [](DeviceSnapshot& s, const py::bytes& data, size_t offset) {
               std::string str = data;
               py::gil_scoped_release release;
               s.copyInHost(str.data(), str.size(), offset);
           },
           py::arg("data"),
           py::arg("offset") = 0)
      .def("copy_out_host",
           [](DeviceSnapshot& s, size_t n, size_t offset) {
               std::vector<uint8_t> out(n);
               {
                   py::gil_scoped_release release;
                   s.copyOutHost(out.data(), n, offset);
               }
               return py::bytes((const char*)out.data(), out.size());
           },
           py::arg("n"),
           py::arg("offset") = 0)
      .def("capture_from_ptr",
           [](DeviceSnapshot& s, uintptr_t ptr) {
               py::gil_scoped_release release;
               s.captureFromDevice((const void*)ptr);
           })
      .def("dirty_pages",
           [](DeviceSnapshot& s, uintptr_t ptr) {
               py::gil_scoped_release release;
               return s.dirtyPages((const void*)ptr);
           })
      .def("diff_xor",
           [](DeviceSnapshot& s, uintptr_t ptr) {
               py::gil_scoped_release release;
               return s.diffXor((const void*)ptr);
           })
      .def("gather_last_diff",
           [](DeviceSnapshot& s) {
               std::vector<uint32_t> pages;
               std::vector<uint8_t> payload;
               {
                   py::gil_scoped_release release;
                   s.gatherLastDiffToHost(pages, payload);
               }
               return py::make_tuple(
                 pages,
                 py::bytes((const char*)payload.data(), payload.size()));
           })
      .def("apply_compact_diff",
           [](DeviceSnapshot& s,
              const std::vector<uint32_t>& pages,
              const py::bytes& payload) {
               std::string data = payload;
               py::gil_scoped_release release;
               s.applyCompactDiffFromHost(
                 pages, (const uint8_t*)data.data(), data.size());
           })
      .def("apply_last_diff", [](DeviceSnapshot& s) {
          py::gil_scoped_release release;
          s.applyLastDiff();
      })
      // Typed merge regions: the packed TypedElems diff of one region
      // (None when no element changed), its merge, the full thread diff
      // under a region list of (offset, length, data_type, operation)
      // tuples, and the join-time queue
      .def("typed_diff",
           [](DeviceSnapshot& s,
              uintptr_t ptr,
              uint32_t offset,
              size_t length,
              SnapshotDataType dataType,
              SnapshotMergeOperation operation) {
               py::gil_scoped_release release;
               return s.typedDiff(
                 (const void*)ptr,
                 SnapshotMergeRegion(offset, length, dataType, operation));
           },
           py::arg("ptr"),
           py::arg("offset"),
           py::arg("length"),
           py::arg("data_type"),
           py::arg("operation"))
      .def("apply_typed_diff",
           [](DeviceSnapshot& s, const SnapshotDiff& diff) {
               py::gil_scoped_release release;
               s.applyTypedDiff(diff);
           })
      .def("diff_with_regions",
           [](DeviceSnapshot& s,
              uintptr_t ptr,
              const std::vector<std::tuple<uint32_t, size_t, int, int>>&
                regions) {
               std::vector<SnapshotMergeRegion> mr;
               for (const auto& [off, len, dt, op] : regions) {
                   mr.emplace_back(off,
                                   len,
                                   (SnapshotDataType)dt,
                                   (SnapshotMergeOperation)op);
               }
               py::gil_scoped_release release;
               return s.diffWithRegions((const void*)ptr, mr);
           },
           py::arg("ptr"),
           py::arg("regions"))
      .def("queue_diff",
           [](DeviceSnapshot& s, const SnapshotDiff& diff) {
               s.queueDiff(diff);
           })
      .def("apply_queued_diffs", [](DeviceSnapshot& s) {
          py::gil_scoped_release release;
          return s.applyQueuedPackedDiffs();
      });

    // The device merge regions registered on this host under the running
    // task's snapshot key, as (offset, length, data_type, operation)
    m.def("executor_device_merge_regions", [] {
        const Message& msg = ExecutorContext::get().getMsg();
        std::vector<std::tuple<uint32_t, size_t, int, int>> out;
        for (const auto& r :
             DeviceSnapshotRegistry::get().getMergeRegions(msg.snapshotKey)) {
            out.emplace_back(
              r.offset, r.length, (int)r.dataType, (int)r.operation);
        }
        return out;
    });
    m.def("device_elementwise_op",
          [](uintptr_t inout,
             uintptr_t in,
             uint64_t count,
             int dtype,
             int op) {
              py::gil_scoped_release release;
              deviceElementwiseOp(
                (void*)inout, (const void*)in, count, dtype, op);
          });

    // Direct famCopyBuffer bandwidth: returns GB/s (2-unit traffic)
    m.def("bench_copy", [](size_t bytes, int iters) {
        py::gil_scoped_release release;
        uint8_t* src = nullptr;
        uint8_t* dst = nullptr;
        if (hipMalloc(&src, bytes) != hipSuccess ||
            hipMalloc(&dst, bytes) != hipSuccess) {
            throw FaabricException("bench_copy alloc failed");
        }
        (void)hipMemset(src, 0x5a, bytes);
        (void)hipDeviceSynchronize();
        // warmup
        (void)famCopyBuffer(src, dst, bytes, nullptr);
        (void)hipDeviceSynchronize();
        int64_t t0 = getEpochMicros();
        for (int i = 0; i < iters; i++) {
            (void)famCopyBuffer(src, dst, bytes, nullptr);
        }
        (void)hipDeviceSynchronize();
        int64_t t1 = getEpochMicros();
        (void)hipFree(src);
        (void)hipFree(dst);
        return 2.0 * bytes * iters / ((t1 - t0) / 1e6) / 1e9;
    }, py::arg("bytes"), py::arg("iters") = 20);

    m.def("bench_snapshot_pipeline",
          &benchSnapshotPipeline,
          py::arg("bytes"),
          py::arg("iters") = 5,
          py::arg("warmup") = 2,
          py::arg("dirty_pct") = 25.0,
          py::arg("device") = 0);
    m.def("fam_fill_random",
          [](uintptr_t ptr, uint64_t bytes, uint64_t seed) {
              py::gil_scoped_release release;
              hipError_t rc =
                famFillRandom((void*)ptr, bytes, seed, nullptr);
              if (rc == hipSuccess) {
                  rc = hipDeviceSynchronize();
              }
              if (rc != hipSuccess) {
                  throw FaabricException("famFillRandom failed");
              }
          });
    // Thin wrappers over the D2D copy and whole-buffer XOR kernels (null
    // stream, synchronised) so they can be driven without an MPI world
    m.def("fam_copy_buffer",
          [](uintptr_t src, uintptr_t dst, uint64_t bytes) {
              py::gil_scoped_release release;
              hipError_t rc = famCopyBuffer(
                (const void*)src, (void*)dst, bytes, nullptr);
              if (rc == hipSuccess) {
                  rc = hipDeviceSynchronize();
              }
              if (rc != hipSuccess) {
                  throw FaabricException("famCopyBuffer failed");
              }
          });
    m.def("fam_xor_buffer",
          [](uintptr_t a, uintptr_t b, uintptr_t out, uint64_t bytes) {
              py::gil_scoped_release release;
              hipError_t rc = famXorBuffer(
                (const void*)a, (const void*)b, (void*)out, bytes, nullptr);
              if (rc == hipSuccess) {
                  rc = hipDeviceSynchronize();
              }
              if (rc != hipSuccess) {
                  throw FaabricException("famXorBuffer failed");
              }
          });
    m.def("fam_touch_pages",
          [](uintptr_t ptr, const std::vector<uint32_t>& pages,
             uint64_t seed) {
              py::gil_scoped_release release;
              uint32_t* pagesDev = nullptr;
              if (hipMalloc(&pagesDev,
                            pages.size() * sizeof(uint32_t)) !=
                  hipSuccess) {
                  throw FaabricException("touch pages alloc failed");
              }
              hipError_t rc =
                hipMemcpy(pagesDev, pages.data(),
                          pages.size() * sizeof(uint32_t),
                          hipMemcpyHostToDevice);
              if (rc == hipSuccess) {
                  rc = famTouchPages((void*)ptr, pagesDev,
                                     (uint32_t)pages.size(), seed,
                                     nullptr);
              }
              if (rc == hipSuccess) {
                  rc = hipDeviceSynchronize();
              }
              (void)hipFree(pagesDev);
              if (rc != hipSuccess) {
                  throw FaabricException("famTouchPages failed");
              }
          });
}

// rt_gather.cpp — the device-resident multi-device frame: peer
// access, rt_assemble_async, rt_gather_async and rt_render_gather_async.
//
// main_cuda.cu:280-339 renders on one device and copies the three planes to
// the host.  Several devices of one node: each renders its cyclic row tiles,
// and the tiles travel device to device over xGMI (peer copies on the
// destination's copy engines: a gather into one device is G-1 point-to-point
// transfers, which is all ncclGather, rccl.h:745, would issue for it inside one
// process), then the assemble kernel un-permutes them into row order.
#include <array>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "rt_host_slots.h"
#include "rt_pack.h"
#include "rt_rccl.h"

using namespace rt;

namespace {

// Peer access of dst to src, enabled once per pair.  Status: 1 = enabled
// (the copy engines read src over xGMI), 0 = not available, refused
// (e.g. hipErrorPeerAccessUnsupported) or switched off with the environment
// variable RT_PEER_ACCESS=0; hipMemcpyPeerAsync then stages the copy through
// the host itself, so the gather still works, only slower.
std::mutex g_peer_mu;
std::vector<std::array<int, 3>> g_peer;      // (dst, src, status)

int enable_peer(int dst, int src)
{
    if (dst == src) return 1;
    std::lock_guard<std::mutex> lk(g_peer_mu);
    for (auto& d : g_peer)
        if (d[0] == dst && d[1] == src) return d[2];
    int status = 0;
    const char* env = std::getenv("RT_PEER_ACCESS");
    int can = 0;
    if (!(env && env[0] == '0') && hipDeviceCanAccessPeer(&can, dst, src) == hipSuccess && can) {
        DeviceGuard g(dst);
        const hipError_t e = hipDeviceEnablePeerAccess(src, 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) status = 1;
        (void)hipGetLastError();     // a refusal must not poison the next call's error check
    }
    g_peer.push_back({dst, src, status});
    return status;
}

// world blocks of rows_per_rank rows (whole tiles of tile_rows) cover the
// H rows of a W-wide frame
int check_gather_geometry(int world, int tile_rows, int rows_per_rank, int W, int H)
{
    if (world < 1 || tile_rows < 1 || rows_per_rank < 0 || W < 1 || H < 1 || rows_per_rank % tile_rows)
        return fail(RT_EINVAL, "bad gather geometry");
    const long long tiles = (H + tile_rows - 1) / tile_rows;
    if ((long long)world * (rows_per_rank / tile_rows) < tiles)
        return fail(RT_EINVAL, "%d ranks x %d tiles < %lld tiles", world, rows_per_rank / tile_rows, tiles);
    return RT_OK;
}

// One plane: slot r's rows_per_rank*W colours (device src_dev[r]) into the
// rank-major staging block r on dst_dev, then assemble into out (W*H).
int gather_plane(int world, const int* src_dev, const rt_color* const* locals, int tile_rows, int rows_per_rank,
                 int W, int H, int dst_dev, rt_color* staging, rt_color* out, hipStream_t st)
{
    const size_t n = (size_t)rows_per_rank * W;
    for (int r = 0; r < world; ++r) {
        if (!locals[r]) return fail(RT_EINVAL, "locals[%d] is NULL", r);
        enable_peer(dst_dev, src_dev[r]);
        const hipError_t e = hipMemcpyPeerAsync(staging + (size_t)r * n, dst_dev, locals[r], src_dev[r],
                                                n * sizeof(rt_color), st);
        if (e != hipSuccess) return fail(RT_EDEVICE, "peer copy %d -> %d: %s", src_dev[r], dst_dev, hipGetErrorString(e));
    }
    return rt_assemble_async(staging, (long long)n, world, tile_rows, rows_per_rank, W, H, out, st);
}

thread_local std::string g_gather_transport = "none";

}  // namespace

extern "C" {

int rt_peer_access(int dst_device, int src_device)
{
    const int n = rt_device_count();
    if (dst_device < 0 || dst_device >= n || src_device < 0 || src_device >= n)
        return fail(RT_EINVAL, "peer pair %d <- %d: %d visible device%s", dst_device, src_device, n, n == 1 ? "" : "s");
    return enable_peer(dst_device, src_device);
}

int rt_assemble_async(const rt_color* gathered, long long rank_stride, int world, int tile_rows, int rows_per_rank,
                      int W, int H, rt_color* out, void* hip_stream)
{
    int rc;
    if (!gathered || !out) return fail(RT_EINVAL, "NULL buffer");
    if ((rc = check_gather_geometry(world, tile_rows, rows_per_rank, W, H))) return rc;
    if (rank_stride == 0) rank_stride = (long long)rows_per_rank * W;
    if (rank_stride < (long long)rows_per_rank * W) return fail(RT_EINVAL, "rank_stride overlaps rank blocks");
    const int e = launch_assemble((const double*)gathered, rank_stride, world, tile_rows, rows_per_rank, W, H,
                                  (double*)out, hip_stream);
    if (e) return fail(RT_EDEVICE, "assemble launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_assemble_packed_async(const unsigned* gathered, long long rank_stride, int world, int tile_rows,
                             int rows_per_rank, int W, int H, rt_color* out, void* hip_stream)
{
    int rc;
    if (!gathered || !out) return fail(RT_EINVAL, "NULL buffer");
    if ((uintptr_t)gathered % 4) return fail(RT_EINVAL, "packed canva is not 4-byte aligned");
    if ((rc = check_gather_geometry(world, tile_rows, rows_per_rank, W, H))) return rc;
    if (rank_stride == 0) rank_stride = (long long)rows_per_rank * W;
    if (rank_stride < (long long)rows_per_rank * W) return fail(RT_EINVAL, "rank_stride overlaps rank blocks");
    const int e = launch_assemble_packed(gathered, rank_stride, world, tile_rows, rows_per_rank, W, H, (double*)out,
                                         hip_stream);
    if (e) return fail(RT_EDEVICE, "assemble launch: %s", hipGetErrorString((hipError_t)e));
    return RT_OK;
}

int rt_gather_async(int world, const int* src_devices, const rt_color* const* locals, int tile_rows,
                    int rows_per_rank, int W, int H, int dst_device, rt_color* out, void* hip_stream)
{
    int rc;
    if (!src_devices || !locals || !out) return fail(RT_EINVAL, "NULL argument");
    if ((rc = check_gather_geometry(world, tile_rows, rows_per_rank, W, H))) return rc;
    DeviceGuard g(dst_device);
    hipStream_t st = (hipStream_t)hip_stream;
    StreamBuffer staging;
    HIP_TRY(staging.alloc((size_t)world * rows_per_rank * W * sizeof(rt_color), st, dst_device));
    return gather_plane(world, src_devices, locals, tile_rows, rows_per_rank, W, H, dst_device, (rt_color*)staging.p,
                        out, st);
}

const char* rt_last_gather_transport(void) { return g_gather_transport.c_str(); }

int rt_render_gather_async(const rt_scene* scene, const rt_params* params, int tile_rows, const rt_frame* frame,
                           void* hip_stream)
{
    int rc;
    if ((rc = validate_scene(scene)) || (rc = validate_params(params))) return rc;
    if (!frame || !frame->canva) return fail(RT_EINVAL, "frame.canva is NULL");
    if (tile_rows < 1) return fail(RT_EINVAL, "tile_rows %d < 1", tile_rows);
    std::vector<int> devs;
    if ((rc = device_list(devs))) return rc;
    const int G = (int)devs.size(), W = params->largeur_image, H = params->hauteur_image;
    // RT_GATHER_RCCL: one rank per device, so the list must not repeat one; the
    // communicators are made (once per list) before anything is enqueued
    // (the tests' stand-in library, rt_rccl.h, takes a list that repeats one)
    const bool packed = (params->gather & RT_GATHER_PACKED_CANVA) != 0;
    const bool rccl = (params->gather & ~RT_GATHER_PACKED_CANVA) == RT_GATHER_RCCL;
    if (rccl) {
        for (int a = 0; a < G; ++a)
            for (int b = a + 1; b < G; ++b)
                if (devs[(size_t)a] == devs[(size_t)b] && !rccl_ranks_may_share_a_device())
                    return fail(RT_EUNSUPPORTED, "RT_GATHER_RCCL needs distinct devices (rt_init's list names device %d "
                                                 "twice; RCCL has one rank per GPU): use RT_GATHER_PEER", devs[(size_t)a]);
        std::string err;
        if (rccl_comms(devs, err)) return fail(RT_EDEVICE, "RCCL: %s", err.c_str());
    }
    const int dst = devs[0];
    const int n_tiles = (((H + tile_rows - 1) / tile_rows) + G - 1) / G;      // per slot (rows >= H skipped)
    const int rows_pr = n_tiles * tile_rows;
    rt_color* outs[4] = {frame->canva, frame->albedo, frame->normal, frame->radiance};
    int nplanes = 0;
    for (rt_color* o : outs) nplanes += o ? 1 : 0;
    const size_t plane = (size_t)rows_pr * W;                            // colours per plane and slot
    if (packed && (long long)plane > kPackMaxPixels)
        return fail(RT_EINVAL, "packed canva: more than 2^30 pixels per slot");
    // RT_GATHER_PACKED_CANVA: the canva travels as one word per pixel, packed by
    // its slot; the other nwide requested planes travel as doubles
    const int nwide = nplanes - (packed ? 1 : 0);
    hipStream_t dst_st = (hipStream_t)hip_stream;

    // 1. every slot renders its tiles on its own device and pooled stream,
    //    after whatever the caller enqueued on hip_stream before this call
    Event go;                                  // outlives the slots, whose streams wait for it
    std::vector<RenderSlot> slots((size_t)G);
    auto planes_of = [&](int q) { return (rt_color*)slots[(size_t)q].buf.p; };
    {
        DeviceGuard g(dst);
        HIP_TRY(go.create());
        HIP_TRY(hipEventRecord(go, dst_st));
    }
    for (int q = 0; q < G && rc == RT_OK; ++q)
        rc = slots[(size_t)q].render(devs[(size_t)q], scene, params, rt_tiling{0, tile_rows, q, G, n_tiles}, H, outs, go,
                                     packed);
    // 2. the destination's stream waits for every slot, gathers each plane over
    //    xGMI and un-permutes it; 3. each slot frees its planes after the copies
    if (rc == RT_OK) {
        DeviceGuard g(dst);
        for (int q = 0; q < G && rc == RT_OK; ++q) {
            const hipError_t e = hipStreamWaitEvent(dst_st, slots[(size_t)q].rendered, 0);
            if (e != hipSuccess) rc = fail(RT_EDEVICE, "wait: %s", hipGetErrorString(e));
        }
        if (rc == RT_OK) {
            StreamBuffer staging_buf;          // freed on dst_st behind the assembles, before `go` is recorded again
            // colours staged per slot: RCCL gathers a slot's wide planes in one block, the
            // peer copies take one plane at a time; the packed words of every slot sit behind
            const size_t per_slot = rccl ? plane * nwide : nwide ? plane : 0;
            const size_t wide_bytes = (size_t)G * per_slot * sizeof(rt_color);
            const hipError_t e = staging_buf.alloc(wide_bytes + (packed ? (size_t)G * plane * sizeof(unsigned) : 0),
                                                   dst_st, dst);
            if (e != hipSuccess) rc = fail(RT_ENOMEM, "gather staging: %s", hipGetErrorString(e));
            rt_color* staging = (rt_color*)staging_buf.p;
            unsigned* words = (unsigned*)((char*)staging_buf.p + wide_bytes);
            const size_t wide0 = packed ? 1 : 0;       // a slot's wide planes start behind its canva when that is packed
            if (rccl && rc == RT_OK) {
                // every slot's wide planes (contiguous in its buffer) in one ncclGather to
                // rank 0, its packed canva in a second one of the same group; rank 0's part
                // on hip_stream (which waited for its render), the others' on their own
                // streams after their renders
                std::vector<GatherPart> parts;
                std::vector<hipStream_t> sst((size_t)G);
                for (int q = 0; q < G; ++q) sst[(size_t)q] = q == 0 ? dst_st : slots[(size_t)q].stream->st;
                if (nwide) {
                    GatherPart w;
                    for (int q = 0; q < G; ++q) w.send.push_back(planes_of(q) + wide0 * plane);
                    w.recv = staging;
                    w.count = per_slot * 3;
                    parts.push_back(w);
                }
                if (packed) {
                    GatherPart c;
                    for (int q = 0; q < G; ++q) c.send.push_back(slots[(size_t)q].packed);
                    c.recv = words;
                    c.count = plane;
                    c.words = true;
                    parts.push_back(c);
                }
                std::string err;
                if (rccl_gather(devs, parts, sst, err)) rc = fail(RT_EDEVICE, "RCCL: %s", err.c_str());
            }
            // the k-th wide plane: assembled from the rank-major staging RCCL
            // filled, or gathered by peer copies and then assembled; a packed
            // canva likewise, by the assemble that widens it
            size_t k = 0;
            for (int pl = 0; pl < 4 && rc == RT_OK; ++pl) {
                if (!outs[pl]) continue;
                if (pl == 0 && packed) {
                    for (int q = 0; q < G && !rccl && rc == RT_OK; ++q) {
                        enable_peer(dst, devs[(size_t)q]);
                        const hipError_t ec = hipMemcpyPeerAsync(words + (size_t)q * plane, dst, slots[(size_t)q].packed,
                                                                 devs[(size_t)q], plane * sizeof(unsigned), dst_st);
                        if (ec != hipSuccess)
                            rc = fail(RT_EDEVICE, "peer copy %d -> %d: %s", devs[(size_t)q], dst, hipGetErrorString(ec));
                    }
                    if (rc == RT_OK)
                        rc = rt_assemble_packed_async(words, (long long)plane, G, tile_rows, rows_pr, W, H, outs[pl], dst_st);
                    continue;
                }
                if (rccl) {
                    rc = rt_assemble_async(staging + k * plane, (long long)per_slot, G, tile_rows, rows_pr, W, H,
                                           outs[pl], dst_st);
                } else {
                    std::vector<const rt_color*> loc((size_t)G);
                    for (int q = 0; q < G; ++q) loc[(size_t)q] = planes_of(q) + (k + wide0) * plane;
                    rc = gather_plane(G, devs.data(), loc.data(), tile_rows, rows_pr, W, H, dst, staging, outs[pl], dst_st);
                }
                ++k;
            }
            if (rc == RT_OK) {
                g_gather_transport = rccl ? "rccl: ncclGather, " + rccl_describe() + ", " + std::to_string(G) + " ranks"
                                          : "peer: hipMemcpyPeerAsync, " + std::to_string(G) + " slots";
                if (packed) g_gather_transport += ", canva 4 B/px";
            }
        }
        if (rc == RT_OK) {
            // the slots free their planes only after the copies that read them
            hipError_t e = hipEventRecord(go, dst_st);            // reused: "the copies are done"
            if (e != hipSuccess) rc = fail(RT_EDEVICE, "gather event: %s", hipGetErrorString(e));
            for (int q = 0; q < G && rc == RT_OK; ++q) {
                DeviceGuard gq(devs[(size_t)q]);
                if ((e = hipStreamWaitEvent(slots[(size_t)q].stream->st, go, 0)) != hipSuccess)
                    rc = fail(RT_EDEVICE, "device %d wait: %s", devs[(size_t)q], hipGetErrorString(e));
            }
        }
    }
    if (rc != RT_OK) {
        // Keep the error message.  Copies already queued on the destination's
        // stream may still read slot planes, and the slots may still render
        // into them: drain both before the slots' destructors hand the memory
        // back.
        {
            DeviceGuard g(dst);
            (void)hipStreamSynchronize(dst_st);
        }
        for (auto& s : slots)
            if (s.stream.ps) {
                DeviceGuard gq(s.stream->device);
                (void)hipStreamSynchronize(s.stream->st);
            }
    }
    return rc;     // on success nothing above waited for the GPU: the slots free their planes in stream order
}

}  // extern "C"

// nnn_batch_snapshot.hip -- whole-batch state images (state_bytes, save_state, load_state) and clone.
// Needs nnn_batch_core.hip (quiesce), create_batch of nnn_batch_create.hip, hold_prepare of nnn_batch_streams.hip, floor_clone of
// nnn_batch_floor.hip and link_clone of nnn_batch_link.hip.
#pragma once

// ---- state snapshots: DenoiseState is Clone in the reference (src/denoise.rs:36) ------------------------------------
struct SnapHeader { uint64_t magic, frame_count, group_count, n_bufs, total, streams; };
constexpr uint64_t kSnapMagic = 0x6e6e6e5f73743032ull;   // "nnn_st02"

extern "C" size_t nnn_batch_state_bytes(const nnn_batch *h)
{
    if (!h) return 0;
    size_t n = sizeof(SnapHeader);
    for (auto &sb : h->state_bufs) n += sb.second;
    return n;
}

extern "C" int nnn_batch_save_state(nnn_batch *h, void *host_dst, size_t dst_bytes)
{
    NNN_RT_LOCK;
    if (!h || !host_dst) return fail("null argument");
    if (int rc = refuse_pending(h, "nnn_batch_save_state")) return rc;
    const size_t need = nnn_batch_state_bytes(h);
    if (dst_bytes < need) return fail("state buffer too small: %zu bytes needed", need);
    if (h->n_held) return fail("nnn_batch_save_state refused: %d streams are held (nnn_batch_hold_streams) and the raw state image has no place for their parked records; resume or export them first", h->n_held);
    if (int rc = quiesce(h)) return rc;
    SnapHeader hd{kSnapMagic, h->frame_count, h->group_count, (uint64_t)h->state_bufs.size(), (uint64_t)need, (uint64_t)h->S};
    char *p = (char *)host_dst;
    memcpy(p, &hd, sizeof(hd));
    p += sizeof(hd);
    for (auto &sb : h->state_bufs) {
        HIPCHK(hipMemcpy(p, sb.first, sb.second, hipMemcpyDeviceToHost));
        p += sb.second;
    }
    return 0;
}

extern "C" int nnn_batch_load_state(nnn_batch *h, const void *host_src, size_t src_bytes)
{
    NNN_RT_LOCK;
    if (!h || !host_src) return fail("null argument");
    if (int rc = refuse_pending(h, "nnn_batch_load_state")) return rc;
    const size_t need = nnn_batch_state_bytes(h);
    SnapHeader hd;
    if (src_bytes < sizeof(hd)) return fail("not a state snapshot");
    memcpy(&hd, host_src, sizeof(hd));
    if (hd.magic != kSnapMagic || hd.n_bufs != h->state_bufs.size() || hd.total != need || hd.streams != (uint64_t)h->S || src_bytes < need)
        return fail("state snapshot does not match this batch (streams / models / max_group_frames / library build)");
    if (h->n_held) return fail("nnn_batch_load_state refused: %d streams are held (nnn_batch_hold_streams) and the raw state image has no place for their parked records; resume them or nnn_batch_reset first", h->n_held);
    if (int rc = quiesce(h)) return rc;
    const char *p = (const char *)host_src + sizeof(hd);
    for (auto &sb : h->state_bufs) {
        HIPCHK(hipMemcpy(sb.first, p, sb.second, hipMemcpyHostToDevice));
        p += sb.second;
    }
    HIPCHK(hipDeviceSynchronize());
    *h->fault_host = 0;
    h->frame_count = hd.frame_count;
    h->group_count = hd.group_count;
    h->prev_pipe = false;
    return 0;
}

extern "C" nnn_batch *nnn_batch_clone(nnn_batch *h)
{
    NNN_RT_LOCK;
    if (!h) { fail("null batch"); return nullptr; }
    if (refuse_pending(h, "nnn_batch_clone")) return nullptr;
    if (quiesce(h)) return nullptr;
    std::vector<const RNNModel *> mp;
    for (const RNNModel &m : h->models) mp.push_back(&m);
    // made as the source was made (not from the environment of now: its depth, ring and kernel forms must match), then set as it is
    nnn_batch *c = create_batch(mp.data(), h->group_streams.data(), (int)h->group_streams.size(), h->device, h->gmax, h->created);
    if (!c) return nullptr;
    bool ok = c->state_bufs.size() == h->state_bufs.size();
    for (size_t i = 0; ok && i < h->state_bufs.size(); i++)
        ok = c->state_bufs[i].second == h->state_bufs[i].second &&
             hipMemcpy(c->state_bufs[i].first, h->state_bufs[i].first, h->state_bufs[i].second, hipMemcpyDeviceToDevice) == hipSuccess;
    if (!ok || hipDeviceSynchronize() != hipSuccess) {
        nnn_batch_destroy(c);
        fail("state copy failed");
        return nullptr;
    }
    if (h->n_held) {   // the same held set and parked records
        ok = hold_prepare(c) == 0 &&
             hipMemcpy(c->park, h->park, (size_t)h->S * NNN_STREAM_STATE_BYTES, hipMemcpyDeviceToDevice) == hipSuccess &&
             hipMemcpy(c->live, h->live, (size_t)h->NT * sizeof(unsigned long long), hipMemcpyDeviceToDevice) == hipSuccess &&
             hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            nnn_batch_destroy(c);
            fail("copy of the parked records failed");
            return nullptr;
        }
        c->held = h->held;
        c->n_held = h->n_held;
    }
    if (floor_clone(c, h) != 0) {   // the same gain floors (configuration travels with a clone)
        nnn_batch_destroy(c);
        fail("copy of the gain floors failed");
        return nullptr;
    }
    link_clone(c, h);   // ... and the same channel link
    c->frame_count = h->frame_count;
    c->group_count = h->group_count;
    c->paths = h->paths;
    if (h->b[0].taps && nnn_batch_set_taps(c, h->b[0].taps) != 0) {
        nnn_batch_destroy(c);
        return nullptr;
    }
    return c;
}

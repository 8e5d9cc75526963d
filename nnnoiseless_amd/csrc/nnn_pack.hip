// nnn_pack.hip -- the file packer (include/nnn_pack.h): files of unequal length through one batch, slots refilled.
// One run = a plan (pack_plan: pure host arithmetic, what nnn_pack_plan returns) walked step by step; one step = the slots' descriptors up
// from page-locked memory -> k_pack_in (the files' spans, converted, into uniformly strided staging rows) -> the batch's ordinary call over
// the rows, in place -> k_pack_out (the frames that belong to a file back to its output range, its VAD values beside them), all on the
// caller's stream, with nnn_batch_reset_streams / nnn_batch_hold_streams between the steps for the slots that change hands.
// Needs struct nnn_batch, fail / HIPCHK, refuse_pending and report_fault (nnn_batch_core.hip), the stream calls (nnn_batch_streams.hip),
// nnn_batch_process_pcm_device (nnn_batch_launch.hip) and pcm_to_i16 (nnn_common.hip).
// ref: src/nnnoiseless.rs:189-227 (the sample conversions), :301-331 (the loop: whole frames only, the first one not written).
#pragma once

#include <algorithm>

#include "../../include/nnn_pack.h"

// ---- the two kernels ---------------------------------------------------------------------------------------------------------------
// The staging is f32 in the batch's own interleaved layout: slot g's row at stage + g * row, frame t of it at t * 480 * C, so a file's
// interleaved frames are one straight copy and the batch reads them with group_stride = row, frame_stride = 480 * C.  A block serves ONE
// slot (blockIdx.x) and 1024 consecutive staging elements of it (blockIdx.y), a thread four of them: on the staging side always one
// 16-byte access, 1 KiB per wave instruction.  On the arena side the four elements lie wherever the file's offset puts them; since a
// thread's first element is a multiple of 4, the address class (mod 16 for 4-byte elements, mod 8 for int16, mod 4 for packed 24-bit) is
// the same for every thread of a block, and the block takes the widest access the class allows: one 16- / 8- / 3 x 4-byte access when
// the span happens to be aligned, 4-byte words for half-aligned int16, else element by element (bytes for 24-bit).  Whole frames are
// multiples of four elements, so the span's end never cuts a thread's four: no head and no tail beside the zero fill.
constexpr int PK_THREADS = 256, PK_VEC = 4, PK_CHUNK = PK_THREADS * PK_VEC;
constexpr int PK_I24 = NNN_PACK_I24, PK_I32 = NNN_PACK_I32, PK_F32_WAV = NNN_PACK_F32_WAV;

struct PackDesc {          // one slot's share of one step (32 bytes)
    long long in_off;      // element of the input arena where the step's part of the slot's file begins
    long long out0;        // element of the output arena staging element 0 of the step belongs at: out_off + (f0 - 1) * 480 * C, f0 = the file's
                           // frame the step begins with (one frame below out_off while f0 == 0: that frame is skipped)
    long long vad0;        // element of the VAD arena of the step's first frame, channel 0: vad_off + f0 * C
    int valid;             // frames of the step that belong to the file; 0 = the slot is idle (held)
    int skip;              // 1 = the step begins with the file's frame 0: processed, not written
};

struct PackArgs {
    const PackDesc *desc;  // [n_slots], this step's
    const char *in;        // the input arena
    char *out;             // the output arena
    float *vad;            // the VAD arena, or null
    float *stage;          // [n_slots][row]
    const float *vstage;   // [n_k][S]: the step's VAD rows as the batch writes them
    long long row;         // floats per staging row: step_frames * 480 * C
    int span;              // staging elements of this step per slot: n_k * 480 * C
    int fe;                // elements per frame: 480 * C
    int S, C;
};

__device__ __forceinline__ long long pk_uniform(long long v)
{
    const int lo = __builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v & 0xffffffffull));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ float pk_s16(unsigned lo16) { return (float)(short)(unsigned short)(lo16 & 0xffffu); }

// four consecutive elements at byte address p, as the floats process_frame takes
template <int FMT> __device__ __forceinline__ float4 pack_load4(const char *p)
{
    const uintptr_t a = (uintptr_t)p;
    float4 v;
    if (FMT == PCM_I16) {
        if ((a & 7) == 0) {
            const uint2 w = *(const uint2 *)p;
            v.x = pk_s16(w.x), v.y = pk_s16(w.x >> 16), v.z = pk_s16(w.y), v.w = pk_s16(w.y >> 16);
        } else if ((a & 3) == 0) {
            const unsigned w0 = ((const unsigned *)p)[0], w1 = ((const unsigned *)p)[1];
            v.x = pk_s16(w0), v.y = pk_s16(w0 >> 16), v.z = pk_s16(w1), v.w = pk_s16(w1 >> 16);
        } else {
            const short *s = (const short *)p;
            v.x = (float)s[0], v.y = (float)s[1], v.z = (float)s[2], v.w = (float)s[3];
        }
    } else if (FMT == PK_I24) {   // little-endian: (float)(sext24 >> 8) is the int16 the sample's upper two bytes make
        if ((a & 3) == 0) {
            const unsigned w0 = ((const unsigned *)p)[0], w1 = ((const unsigned *)p)[1], w2 = ((const unsigned *)p)[2];
            v.x = pk_s16(w0 >> 8), v.y = pk_s16(w1), v.z = pk_s16((w1 >> 24) | (w2 << 8)), v.w = pk_s16(w2 >> 16);
        } else {
            const unsigned char *b = (const unsigned char *)p;
            v.x = pk_s16((unsigned)b[1] | (unsigned)b[2] << 8), v.y = pk_s16((unsigned)b[4] | (unsigned)b[5] << 8);
            v.z = pk_s16((unsigned)b[7] | (unsigned)b[8] << 8), v.w = pk_s16((unsigned)b[10] | (unsigned)b[11] << 8);
        }
    } else if (FMT == PK_I32) {
        if ((a & 15) == 0) {
            const uint4 w = *(const uint4 *)p;
            v.x = pk_s16(w.x >> 16), v.y = pk_s16(w.y >> 16), v.z = pk_s16(w.z >> 16), v.w = pk_s16(w.w >> 16);
        } else {
            const unsigned *w = (const unsigned *)p;
            v.x = pk_s16(w[0] >> 16), v.y = pk_s16(w[1] >> 16), v.z = pk_s16(w[2] >> 16), v.w = pk_s16(w[3] >> 16);
        }
    } else {
        if ((a & 15) == 0) v = *(const float4 *)p;
        else {
            const float *f = (const float *)p;
            v.x = f[0], v.y = f[1], v.z = f[2], v.w = f[3];
        }
        if (FMT == PK_F32_WAV) v.x = v.x * 32767.0f, v.y = v.y * 32767.0f, v.z = v.z * 32767.0f, v.w = v.w * 32767.0f;
    }
    return v;
}

template <int FMT> __global__ void __launch_bounds__(PK_THREADS) k_pack_in(PackArgs a)
{
    const int slot = blockIdx.x;
    const PackDesc *d = a.desc + slot;
    const int valid = __builtin_amdgcn_readfirstlane(d->valid);
    if (valid == 0) return;   // an idle slot: held in the batch, its staging row is neither read nor written
    const int e = (int)(blockIdx.y * PK_CHUNK + threadIdx.x * PK_VEC);
    if (e >= a.span) return;
    const long long in_off = pk_uniform(d->in_off);
    constexpr int ES = FMT == PCM_I16 ? 2 : FMT == PK_I24 ? 3 : 4;
    float4 v;
    v.x = v.y = v.z = v.w = 0.0f;   // behind the file's last whole frame the slot is fed zeros
    if (e < valid * a.fe) v = pack_load4<FMT>(a.in + (in_off + e) * ES);
    *(float4 *)(a.stage + (long long)slot * a.row + e) = v;
}

template <int FMT> __global__ void __launch_bounds__(PK_THREADS) k_pack_out(PackArgs a)
{
    const int slot = blockIdx.x;
    const PackDesc *d = a.desc + slot;
    const int valid = __builtin_amdgcn_readfirstlane(d->valid);
    if (valid == 0) return;
    const int skip = __builtin_amdgcn_readfirstlane(d->skip);
    if (blockIdx.y == 0 && a.vad) {   // every processed frame of the file has a VAD value, the first one included
        const long long vad0 = pk_uniform(d->vad0);
        for (int i = threadIdx.x; i < valid * a.C; i += PK_THREADS) {
            const int f = i / a.C, c = i - f * a.C;
            a.vad[vad0 + i] = a.vstage[(long long)f * a.S + slot * a.C + c];
        }
    }
    const int e = (int)(blockIdx.y * PK_CHUNK + threadIdx.x * PK_VEC);
    if (e >= valid * a.fe || (skip && e < a.fe)) return;   // padded frames and the file's frame 0 are not written
    const long long out0 = pk_uniform(d->out0);
    const float4 v = *(const float4 *)(a.stage + (long long)slot * a.row + e);
    if (FMT == PCM_I16) {
        short *q = (short *)a.out + (out0 + e);
        const unsigned s0 = (unsigned short)pcm_to_i16(v.x), s1 = (unsigned short)pcm_to_i16(v.y), s2 = (unsigned short)pcm_to_i16(v.z),
                       s3 = (unsigned short)pcm_to_i16(v.w);
        const uintptr_t qa = (uintptr_t)q;
        if ((qa & 7) == 0) {
            uint2 w;
            w.x = s0 | s1 << 16, w.y = s2 | s3 << 16;
            *(uint2 *)q = w;
        } else if ((qa & 3) == 0) {
            ((unsigned *)q)[0] = s0 | s1 << 16;
            ((unsigned *)q)[1] = s2 | s3 << 16;
        } else {
            q[0] = (short)s0, q[1] = (short)s1, q[2] = (short)s2, q[3] = (short)s3;
        }
    } else {
        float *q = (float *)a.out + (out0 + e);
        if (((uintptr_t)q & 15) == 0) *(float4 *)q = v;
        else q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
    }
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
// The rule of include/nnn_pack.h, as data: per file its slot and first step, per step its frames, the summary.  nnn_pack_plan returns it,
// nnn_pack_run_device walks it.
static int pack_plan(int n_slots, int step_frames, const uint64_t *file_frames, int n_files, int32_t *slot_of_file, int32_t *first_step_of_file,
                     int64_t summary[8], std::vector<int32_t> *step_len)
{
    if (n_slots < 1) return fail("nnn_pack_plan: n_slots must be at least 1");
    if (step_frames < 1) return fail("nnn_pack_plan: step_frames must be at least 1");
    if (n_files < 0 || (n_files > 0 && !file_frames)) return fail("nnn_pack_plan: bad file list");
    if (!summary) return fail("nnn_pack_plan: null summary");
    for (int i = 0; i < n_files; i++)
        if (file_frames[i] >= (1ull << 31)) return fail("nnn_pack_plan: file %d has %llu frames, more than a plan counts", i, (unsigned long long)file_frames[i]);
    for (int i = 0; i < n_files; i++) {
        if (slot_of_file) slot_of_file[i] = -1;
        if (first_step_of_file) first_step_of_file[i] = -1;
    }
    std::vector<int64_t> rem((size_t)n_slots, 0);
    int64_t steps = 0, useful = 0, padded = 0, held_steps = 0, held_frames = 0, launched = 0, placed = 0, max_pad = 0;
    int next = 0;
    if (step_len) step_len->clear();
    for (;;) {
        int64_t longest = 0;
        for (int g = 0; g < n_slots; g++) {   // free slots take the next files in list order, lowest slot first
            if (rem[(size_t)g] == 0) {
                while (next < n_files && file_frames[next] == 0) next++;
                if (next < n_files) {
                    rem[(size_t)g] = (int64_t)file_frames[next];
                    if (slot_of_file) slot_of_file[next] = g;
                    if (first_step_of_file) first_step_of_file[next] = (int32_t)steps;
                    next++, placed++;
                }
            }
            longest = std::max(longest, rem[(size_t)g]);
        }
        if (longest == 0) break;
        const int64_t n_k = std::min<int64_t>(step_frames, longest);
        for (int g = 0; g < n_slots; g++) {
            int64_t &r = rem[(size_t)g];
            if (r > 0) {
                const int64_t used = std::min(r, n_k);
                useful += used, padded += n_k - used, max_pad = std::max(max_pad, n_k - used);
                r -= used;
            } else {
                held_steps += 1, held_frames += n_k;
            }
        }
        launched += n_k * n_slots;
        if (step_len) step_len->push_back((int32_t)n_k);
        if (++steps >= (1ll << 31) - 1) return fail("nnn_pack_plan: more steps than a plan counts");
    }
    summary[0] = steps, summary[1] = useful, summary[2] = padded, summary[3] = held_steps, summary[4] = launched, summary[5] = held_frames;
    summary[6] = placed, summary[7] = max_pad;
    return 0;
}

extern "C" int nnn_pack_plan(int n_slots, int step_frames, const uint64_t *file_frames, int n_files, int32_t *slot_of_file,
                             int32_t *first_step_of_file, int64_t summary[8])
{
    return pack_plan(n_slots, step_frames, file_frames, n_files, slot_of_file, first_step_of_file, summary, nullptr);
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
constexpr int PK_PIN = 4;   // page-locked descriptor tables: one is written again only after its event says the copy out of it is done

struct nnn_pack {
    nnn_batch *b = nullptr;
    int S = 0, C = 1, n_slots = 0, step = 0, device = 0;   // (its own copies: destroy must not look into a batch that may be gone)
    float *stage = nullptr;         // device [n_slots][step * 480 * C]: a step's frames, denoised in place
    float *vstage = nullptr;        // device [step][S]
    PackDesc *desc = nullptr;       // device [n_slots]: the current step's table (steps are in order on one stream)
    struct Pin {
        PackDesc *p = nullptr;      // page-locked [n_slots]
        hipEvent_t ev = nullptr;
        bool busy = false;
    } pin[PK_PIN];
    int pin_next = 0;
    hipEvent_t ev_last = nullptr;   // end of the most recent run, on the stream it was made on
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    int64_t summary[8] = {};
    char *h_in = nullptr, *h_out = nullptr;   // device arenas of the host variant (made on first use, grow only)
    float *h_vad = nullptr;
    size_t h_in_cap = 0, h_out_cap = 0, h_vad_cap = 0;
};

static int pack_elem_bytes(int fmt, bool input)
{
    if (fmt == PCM_F32) return 4;
    if (fmt == PCM_I16) return 2;
    if (input && fmt == PK_I24) return 3;
    if (input && (fmt == PK_I32 || fmt == PK_F32_WAV)) return 4;
    return 0;
}

extern "C" void nnn_pack_destroy(nnn_pack *p)
{
    if (!p) return;
    NNN_RT_LOCK;
    hipSetDevice(p->device);
    if (p->have_last) hipEventSynchronize(p->ev_last);
    for (auto &t : p->pin) {
        if (t.busy) hipEventSynchronize(t.ev);
        if (t.p) hipHostFree(t.p);
        if (t.ev) hipEventDestroy(t.ev);
    }
    hipFree(p->stage); hipFree(p->vstage); hipFree(p->desc);
    hipFree(p->h_in); hipFree(p->h_out); hipFree(p->h_vad);
    if (p->ev_last) hipEventDestroy(p->ev_last);
    delete p;
}

extern "C" nnn_pack *nnn_pack_create(nnn_batch *b, int channels, int step_frames)
{
    if (!b) { fail("nnn_pack_create: null batch"); return nullptr; }
    if (channels < 1 || b->S % channels) { fail("nnn_pack_create: n_streams (%d) is not a multiple of channels (%d)", b->S, channels); return nullptr; }
    if (step_frames < 0 || step_frames > b->gmax) {
        fail("nnn_pack_create: step_frames = %d outside [0, nnn_batch_max_group_frames = %d]", step_frames, b->gmax);
        return nullptr;
    }
    if (b->groups.size() > 1) { fail("nnn_pack_create: the batch has %zu model groups; a file may land in any slot, so a packer needs one model", b->groups.size()); return nullptr; }
    if ((long long)(step_frames ? step_frames : b->gmax) * FRAME * channels > 65535ll * PK_CHUNK) {
        fail("nnn_pack_create: %d channels make a step's rows longer than a launch covers", channels);
        return nullptr;
    }
    if (nnn_batch_hold_streams(b, nullptr, 0)) return nullptr;   // the batch's first (empty) hold allocates: now, not in the middle of a run
    NNN_RT_LOCK;
    if (hipSetDevice(b->device) != hipSuccess) { fail("nnn_pack_create: no such HIP device"); return nullptr; }
    nnn_pack *p = new nnn_pack();
    p->b = b;
    p->S = b->S, p->C = channels, p->n_slots = b->S / channels, p->step = step_frames ? step_frames : b->gmax, p->device = b->device;
    bool ok = true;
    auto dev = [&](auto **q, size_t bytes) { ok = ok && hipMalloc((void **)q, bytes ? bytes : 4) == hipSuccess && hipMemset(*q, 0, bytes) == hipSuccess; };
    dev(&p->stage, (size_t)p->S * p->step * FRAME * sizeof(float));
    dev(&p->vstage, (size_t)p->S * p->step * sizeof(float));
    dev(&p->desc, (size_t)p->n_slots * sizeof(PackDesc));
    for (auto &t : p->pin)
        ok = ok && hipHostMalloc((void **)&t.p, (size_t)p->n_slots * sizeof(PackDesc), hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&t.ev, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&p->ev_last, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the memsets above are on the legacy stream; the runs are on non-blocking ones)
    if (!ok) {
        nnn_pack_destroy(p);
        fail("nnn_pack_create: allocation failed");
        return nullptr;
    }
    return p;
}

extern "C" int nnn_pack_last_summary(const nnn_pack *p, int64_t summary[8])
{
    if (!p || !summary) return fail("null argument");
    memcpy(summary, p->summary, sizeof(p->summary));
    return 0;
}

template <bool IN> static void pack_launch(const nnn_pack *p, const PackArgs &a, int fmt, hipStream_t st)
{
    void (*k)(PackArgs);
    if (IN) k = fmt == PCM_I16 ? k_pack_in<PCM_I16> : fmt == PK_I24 ? k_pack_in<PK_I24> : fmt == PK_I32 ? k_pack_in<PK_I32> : fmt == PK_F32_WAV ? k_pack_in<PK_F32_WAV> : k_pack_in<PCM_F32>;
    else k = fmt == PCM_I16 ? k_pack_out<PCM_I16> : k_pack_out<PCM_F32>;
    hipLaunchKernelGGL(k, dim3((unsigned)p->n_slots, (unsigned)((a.span + PK_CHUNK - 1) / PK_CHUNK)), dim3(PK_THREADS), 0, st, a);
}

// the streams of a list of slots, for the batch's stream calls
static void pack_streams(const nnn_pack *p, const std::vector<int> &slots, std::vector<int> &streams)
{
    streams.clear();
    for (int g : slots)
        for (int c = 0; c < p->C; c++) streams.push_back(g * p->C + c);
}

extern "C" int nnn_pack_run_device(nnn_pack *p, const void *d_in, uint64_t in_elems, int in_format, void *d_out, uint64_t out_elems, int out_format,
                                   float *d_vad, uint64_t vad_elems, const nnn_pack_file *files, int n_files, void *hip_stream)
{
    if (!p) return fail("null packer");
    nnn_batch *b = p->b;
    // ---- everything that can be refused, before anything is enqueued
    if (n_files < 0) return fail("nnn_pack_run: n_files = %d", n_files);
    if (!d_in || !d_out) return fail("nnn_pack_run: null arena");
    if (!files) return fail("nnn_pack_run: null file list");
    const int es_in = pack_elem_bytes(in_format, true), es_out = pack_elem_bytes(out_format, false);
    if (!es_in) return fail("nnn_pack_run: unknown input format %d (NNN_PCM_F32, NNN_PCM_I16, NNN_PACK_I24, NNN_PACK_I32, NNN_PACK_F32_WAV)", in_format);
    if (!es_out) return fail("nnn_pack_run: unknown output format %d (NNN_PCM_F32 or NNN_PCM_I16)", out_format);
    if (((uintptr_t)d_out % (uintptr_t)es_out) || (es_in != 3 && ((uintptr_t)d_in % (uintptr_t)es_in)) || ((uintptr_t)d_vad & 3))
        return fail("nnn_pack_run: an arena is not aligned to its element size");
    const uint64_t C = (uint64_t)p->C, FE = (uint64_t)FRAME * C;
    std::vector<uint64_t> frames((size_t)n_files);
    for (int i = 0; i < n_files; i++) {
        const nnn_pack_file &f = files[i];
        const uint64_t F = f.n_frames_samples / FRAME;
        frames[(size_t)i] = F;
        if (f.in_off > in_elems || f.n_frames_samples > (in_elems - f.in_off) / C)
            return fail("nnn_pack_run: file %d: its input span leaves the arena (%llu + %llu x %d elements of %llu)", i, (unsigned long long)f.in_off,
                        (unsigned long long)f.n_frames_samples, p->C, (unsigned long long)in_elems);
        if (F >= (1ull << 31)) return fail("nnn_pack_run: file %d is longer than a run counts", i);
        if (F >= 1 && (f.out_off > out_elems || F - 1 > (out_elems - f.out_off) / FE))
            return fail("nnn_pack_run: file %d: its output span leaves the arena (%llu + %llu elements of %llu)", i, (unsigned long long)f.out_off,
                        (unsigned long long)((F - 1) * FE), (unsigned long long)out_elems);
        if (d_vad && F >= 1 && (f.vad_off > vad_elems || F > (vad_elems - f.vad_off) / C))
            return fail("nnn_pack_run: file %d: its VAD span leaves the arena (%llu + %llu values of %llu)", i, (unsigned long long)f.vad_off,
                        (unsigned long long)(F * C), (unsigned long long)vad_elems);
    }
    if (b->S != p->S || b->S % p->C) return fail("nnn_pack_run: channels (%d) does not divide the batch's streams (%d)", p->C, b->S);
    if (p->step < 1 || p->step > b->gmax) return fail("nnn_pack_run: step_frames = %d outside [1, %d]", p->step, b->gmax);
    if (b->groups.size() > 1) return fail("nnn_pack_run: the batch has more than one model group");
    if (b->n_held > 0) return fail("nnn_pack_run refused: %d streams of the batch are held; a run holds and releases idle slots itself", b->n_held);
    if (int rc = refuse_pending(b, "nnn_pack_run")) return rc;
    if (int rc = report_fault(b)) return rc;
    if (b->paths.inputs_ready) return fail("nnn_pack_run refused: the batch is under nnn_batch_set_inputs_ready(b, 1), and the frames it reads are produced by this call");
    std::vector<int32_t> slot_of((size_t)n_files), first_of((size_t)n_files), step_len;
    int64_t sum[8];
    if (int rc = pack_plan(p->n_slots, p->step, frames.data(), n_files, slot_of.data(), first_of.data(), sum, &step_len)) return rc;
    // ---- the walk
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->stream;
    if (p->have_last && p->last_stream != st) HIPCHK(hipStreamWaitEvent(st, p->ev_last, 0));
    struct Slot { int file = -1; int64_t done = 0; bool held = false, used = false; };
    std::vector<Slot> slots((size_t)p->n_slots);
    std::vector<int> take, idle, streams;
    nnn_pcm_layout L = {};
    L.format = NNN_PCM_F32, L.channels = p->C, L.discard_first = 0;
    L.group_stride = (size_t)p->step * FE, L.frame_stride = (size_t)FE;
    int next = 0;
    for (size_t k = 0; k < step_len.size(); k++) {
        const int n_k = step_len[k];
        take.clear(), idle.clear();
        for (; next < n_files && (first_of[(size_t)next] < 0 || first_of[(size_t)next] == (int32_t)k); next++) {
            if (first_of[(size_t)next] < 0) continue;
            Slot &s = slots[(size_t)slot_of[(size_t)next]];
            s.file = next, s.done = 0, s.used = true;
            take.push_back(slot_of[(size_t)next]);
        }
        for (int g = 0; g < p->n_slots; g++)
            if (slots[(size_t)g].file < 0 && !slots[(size_t)g].held) slots[(size_t)g].held = true, idle.push_back(g);
        if (!take.empty()) {    // a slot starts every file from the freshly-created state
            std::sort(take.begin(), take.end());
            pack_streams(p, take, streams);
            if (int rc = nnn_batch_reset_streams(b, streams.data(), (int)streams.size())) return rc;
        }
        if (!idle.empty()) {    // no file left for these: held for the rest of the run
            pack_streams(p, idle, streams);
            if (int rc = nnn_batch_hold_streams(b, streams.data(), (int)streams.size())) return rc;
        }
        nnn_pack::Pin &pin = p->pin[p->pin_next];
        if (pin.busy) {
            HIPCHK(hipEventSynchronize(pin.ev));   // (the copy out of this table, PK_PIN steps back)
            pin.busy = false;
        }
        for (int g = 0; g < p->n_slots; g++) {
            Slot &s = slots[(size_t)g];
            PackDesc &d = pin.p[g];
            d = PackDesc();
            if (s.file < 0) continue;
            const nnn_pack_file &f = files[s.file];
            const int64_t left = (int64_t)frames[(size_t)s.file] - s.done, valid = std::min<int64_t>(left, n_k);
            d.in_off = (long long)(f.in_off + (uint64_t)s.done * FE);
            d.out0 = (long long)f.out_off + (s.done - 1) * (long long)FE;
            d.vad0 = (long long)(f.vad_off + (uint64_t)s.done * C);
            d.valid = (int)valid;
            d.skip = s.done == 0 ? 1 : 0;
            s.done += valid;
            if (s.done == (int64_t)frames[(size_t)s.file]) s.file = -1;   // free from the next step on
        }
        HIPCHK(hipMemcpyAsync(p->desc, pin.p, (size_t)p->n_slots * sizeof(PackDesc), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(pin.ev, st));
        pin.busy = true;
        p->pin_next = (p->pin_next + 1) % PK_PIN;
        PackArgs a = {};
        a.desc = p->desc, a.in = (const char *)d_in, a.out = (char *)d_out, a.vad = d_vad, a.stage = p->stage, a.vstage = p->vstage;
        a.row = (long long)p->step * (long long)FE, a.span = n_k * (int)FE, a.fe = (int)FE, a.S = p->S, a.C = p->C;
        pack_launch<true>(p, a, in_format, st);
        HIPCHK(hipGetLastError());
        if (int rc = nnn_batch_process_pcm_device(b, p->stage, p->stage, d_vad ? p->vstage : nullptr, n_k, &L, st)) return rc;
        pack_launch<false>(p, a, out_format, st);
        HIPCHK(hipGetLastError());
    }
    if (!step_len.empty()) {   // the batch leaves the run with nothing held and every slot it used fresh
        idle.clear(), take.clear();
        for (int g = 0; g < p->n_slots; g++) {
            if (slots[(size_t)g].held) idle.push_back(g);
            if (slots[(size_t)g].used) take.push_back(g);
        }
        if (!idle.empty()) {
            pack_streams(p, idle, streams);
            if (int rc = nnn_batch_resume_streams(b, streams.data(), (int)streams.size())) return rc;
        }
        pack_streams(p, take, streams);
        if (int rc = nnn_batch_reset_streams(b, streams.data(), (int)streams.size())) return rc;
        // (the stream calls run on the batch's own stream, ordered behind the last step by the batch; the caller's stream sees them done)
        if (st != b->stream && b->have_last) HIPCHK(hipStreamWaitEvent(st, b->ev_last, 0));
    }
    HIPCHK(hipEventRecord(p->ev_last, st));
    p->last_stream = st;
    p->have_last = true;
    memcpy(p->summary, sum, sizeof(sum));
    for (int i : {1, 2, 3, 4, 5}) p->summary[i] *= p->C;
    return 0;
}

extern "C" int nnn_pack_debug_kernels(nnn_pack *p, int which, const void *d_in, int in_format, void *d_out, int out_format, int n_frames, int reps,
                                      void *hip_stream)
{
    if (!p) return fail("null packer");
    if (which != 0 && which != 1) return fail("nnn_pack_debug_kernels: which must be 0 (k_pack_in) or 1 (k_pack_out)");
    if (n_frames < 1 || n_frames > p->step || reps < 0) return fail("nnn_pack_debug_kernels: n_frames outside [1, %d] or negative reps", p->step);
    if (which == 0 ? !d_in || !pack_elem_bytes(in_format, true) : !d_out || !pack_elem_bytes(out_format, false))
        return fail("nnn_pack_debug_kernels: null arena or unknown format");
    nnn_batch *b = p->b;
    HIPCHK(hipSetDevice(b->device));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : b->stream;
    if (p->have_last && p->last_stream != st) HIPCHK(hipStreamWaitEvent(st, p->ev_last, 0));
    HIPCHK(hipStreamSynchronize(st));
    nnn_pack::Pin &pin = p->pin[p->pin_next];
    if (pin.busy) HIPCHK(hipEventSynchronize(pin.ev));
    const long long FE = (long long)FRAME * p->C;
    for (int g = 0; g < p->n_slots; g++) {
        PackDesc &d = pin.p[g];
        d = PackDesc();
        d.in_off = d.out0 = (long long)g * n_frames * FE;
        d.valid = n_frames;
    }
    HIPCHK(hipMemcpyAsync(p->desc, pin.p, (size_t)p->n_slots * sizeof(PackDesc), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(pin.ev, st));
    pin.busy = true;
    p->pin_next = (p->pin_next + 1) % PK_PIN;
    PackArgs a = {};
    a.desc = p->desc, a.in = (const char *)d_in, a.out = (char *)d_out, a.vad = nullptr, a.stage = p->stage, a.vstage = p->vstage;
    a.row = (long long)p->step * FE, a.span = n_frames * (int)FE, a.fe = (int)FE, a.S = p->S, a.C = p->C;
    for (int r = 0; r < reps; r++) {
        if (which == 0) pack_launch<true>(p, a, in_format, st);
        else pack_launch<false>(p, a, out_format, st);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev_last, st));
    p->last_stream = st;
    p->have_last = true;
    return 0;
}

extern "C" int nnn_pack_run_host(nnn_pack *p, const void *in, uint64_t in_elems, int in_format, void *out, uint64_t out_elems, int out_format,
                                 float *vad, uint64_t vad_elems, const nnn_pack_file *files, int n_files)
{
    if (!p) return fail("null packer");
    if (!in || !out) return fail("nnn_pack_run: null arena");
    const int es_in = pack_elem_bytes(in_format, true), es_out = pack_elem_bytes(out_format, false);
    if (!es_in) return fail("nnn_pack_run: unknown input format %d (NNN_PCM_F32, NNN_PCM_I16, NNN_PACK_I24, NNN_PACK_I32, NNN_PACK_F32_WAV)", in_format);
    if (!es_out) return fail("nnn_pack_run: unknown output format %d (NNN_PCM_F32 or NNN_PCM_I16)", out_format);
    nnn_batch *b = p->b;
    HIPCHK(hipSetDevice(b->device));
    const size_t in_bytes = (size_t)in_elems * es_in, out_bytes = (size_t)out_elems * es_out, vad_bytes = vad ? (size_t)vad_elems * sizeof(float) : 0;
    auto room = [&](auto *&q, size_t &cap, size_t bytes) -> int {
        if (bytes <= cap) return 0;
        NNN_RT_LOCK;
        if (int rc = quiesce(b)) return rc;
        if (p->have_last) HIPCHK(hipEventSynchronize(p->ev_last));
        HIPCHK(hipFree(q));
        q = nullptr, cap = 0;
        HIPCHK(hipMalloc((void **)&q, bytes + bytes / 2));
        cap = bytes + bytes / 2;
        return 0;
    };
    if (int rc = room(p->h_in, p->h_in_cap, std::max<size_t>(in_bytes, 16))) return rc;
    if (int rc = room(p->h_out, p->h_out_cap, std::max<size_t>(out_bytes, 16))) return rc;
    if (int rc = room(p->h_vad, p->h_vad_cap, std::max<size_t>(vad_bytes, 16))) return rc;
    hipStream_t st = b->stream;
    if (in_bytes) HIPCHK(hipMemcpyAsync(p->h_in, in, in_bytes, hipMemcpyHostToDevice, st));
    if (out_bytes) HIPCHK(hipMemcpyAsync(p->h_out, out, out_bytes, hipMemcpyHostToDevice, st));   // (what lies outside the files' ranges comes back as it was)
    if (vad_bytes) HIPCHK(hipMemcpyAsync(p->h_vad, vad, vad_bytes, hipMemcpyHostToDevice, st));
    const int rc = nnn_pack_run_device(p, p->h_in, in_elems, in_format, p->h_out, out_elems, out_format, vad ? p->h_vad : nullptr, vad_elems, files,
                                       n_files, st);
    if (rc) {
        hipStreamSynchronize(st);   // (a refusal enqueued nothing: only the uploads above are waited for)
        return rc;
    }
    if (out_bytes) HIPCHK(hipMemcpyAsync(out, p->h_out, out_bytes, hipMemcpyDeviceToHost, st));
    if (vad_bytes) HIPCHK(hipMemcpyAsync(vad, p->h_vad, vad_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

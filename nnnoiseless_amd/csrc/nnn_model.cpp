// nnn_model.cpp -- .rnn model container: parser with the reference's validation rules, the
// built-in weights, the packing the RNN kernels consume (bf16 weights in MFMA B-fragment order, f32 biases), and the
// nnn_model_* entry points of include/nnn_batch.h.
#include "nnn_model.h"

#include <assert.h>
#include <stdio.h>
#include <string.h>

#include "../../include/nnn_batch.h"

int nnn_set_error(const char *msg);   // nnn_batch_core.hip

// The built-in model is the reference's src/weights.rnn (BSD-3-Clause, (c) Mozilla / Xiph / J. Neeman),
// shipped as data in nnnoiseless_amd/data/weights.rnn and linked in verbatim
// (reference: include_bytes!("weights.rnn"), src/rnn.rs:237).
#ifndef NNN_WEIGHTS_PATH
#error "build with -DNNN_WEIGHTS_PATH=\"/abs/path/to/weights.rnn\""
#endif
__asm__(".section .rodata\n"
        ".global nnn_builtin_weights_begin\n"
        ".balign 16\n"
        "nnn_builtin_weights_begin:\n"
        ".incbin \"" NNN_WEIGHTS_PATH "\"\n"
        ".global nnn_builtin_weights_end\n"
        "nnn_builtin_weights_end:\n"
        ".byte 0\n"
        ".text\n");
extern "C" const uint8_t nnn_builtin_weights_begin[];
extern "C" const uint8_t nnn_builtin_weights_end[];

const uint8_t *nnn_builtin_weights(size_t *len)
{
    *len = (size_t)(nnn_builtin_weights_end - nnn_builtin_weights_begin);
    return nnn_builtin_weights_begin;
}

namespace {
struct Cursor {
    const int8_t *base;
    size_t pos, len;
    size_t left() const { return len - pos; }
};

// three header bytes: nb_inputs, nb_neurons (non-negative i8), activation in {0,1,2}; ref: src/rnn.rs:128-152
bool read_header(Cursor &c, int &nin, int &nout, int &act)
{
    if (c.left() < 3) return false;
    const int8_t *b = c.base + c.pos;
    if (b[0] < 0 || b[1] < 0 || b[2] < 0 || b[2] > 2) return false;
    nin = b[0]; nout = b[1]; act = b[2];
    c.pos += 3;
    return true;
}
bool take(Cursor &c, size_t n, size_t &ofs)
{
    if (c.left() < n) return false;
    ofs = c.pos;
    c.pos += n;
    return true;
}
bool read_dense(Cursor &c, NnnDense &l)  // ref: src/rnn.rs:145-164
{
    return read_header(c, l.nb_inputs, l.nb_neurons, l.activation) &&
           take(c, (size_t)l.nb_inputs * l.nb_neurons, l.weights) && take(c, (size_t)l.nb_neurons, l.bias);
}
bool read_gru(Cursor &c, NnnGru &l)  // ref: src/rnn.rs:166-187
{
    if (!read_header(c, l.nb_inputs, l.nb_neurons, l.activation)) return false;
    size_t n = (size_t)l.nb_neurons;
    return take(c, 3 * n * (size_t)l.nb_inputs, l.weights) && take(c, 3 * n * n, l.rec) && take(c, 3 * n, l.bias);
}
}  // namespace

RNNModel *nnn_model_parse(const uint8_t *bytes, size_t len)
{
    RNNModel *m = new RNNModel();
    m->blob.assign((const int8_t *)bytes, (const int8_t *)bytes + len);
    Cursor c{m->blob.data(), 0, len};
    bool ok = read_dense(c, m->input_dense) && read_gru(c, m->vad_gru) && read_gru(c, m->noise_gru) &&
              read_gru(c, m->denoise_gru) && read_dense(c, m->denoise_output) && read_dense(c, m->vad_output);
    ok = ok && c.left() == 0;                                                                   // :196-198
    ok = ok && m->input_dense.nb_inputs == 42 && m->denoise_output.nb_neurons == 22 &&
         m->vad_output.nb_neurons == 1;                                                         // :204-209
    ok = ok && m->input_dense.nb_neurons == m->vad_gru.nb_inputs &&
         m->vad_gru.nb_neurons == m->vad_output.nb_inputs;                                      // :210-213
    ok = ok && 42 + m->input_dense.nb_neurons + m->vad_gru.nb_neurons == m->noise_gru.nb_inputs;   // :214-216
    ok = ok && 42 + m->vad_gru.nb_neurons + m->noise_gru.nb_neurons == m->denoise_gru.nb_inputs;   // :217-219
    ok = ok && m->denoise_gru.nb_neurons == m->denoise_output.nb_inputs;                        // :220-222
    if (!ok) {
        delete m;
        return nullptr;
    }
    return m;
}

namespace {
inline int pad_to(int x, int m) { return (x + m - 1) / m * m; }
inline uint16_t bf16_of_int(int v)  // |v| <= 128: exact
{
    float f = (float)v;
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}

// Appends GEMM operand `g` of the plan in fragment order [neuron block][gate][k-step][lane][8]:
// element = W[colmap(k)][gate * n + neuron], k = kbase + 32 ks + 8 (lane >> 4) + e, neuron = 16 nb + (lane & 15).
template <class ColMap>
void pack_gemm(std::vector<uint16_t> &wq, const nnn::GemmDesc &g, const int8_t *W, int row_stride, int n, ColMap colmap)
{
    assert(wq.size() == (size_t)g.wofs * 8);
    const int nb = pad_to(n, 16) / 16;
    for (int b = 0; b < nb; b++)
        for (int gate = 0; gate < g.ngates; gate++)
            for (int ks = 0; ks < g.ksteps; ks++)
                for (int lane = 0; lane < 64; lane++)
                    for (int e = 0; e < 8; e++) {
                        int k = g.kbase + 32 * ks + 8 * (lane >> 4) + e, neuron = 16 * b + (lane & 15);
                        int row = colmap(k);
                        int v = (row >= 0 && neuron < n) ? W[(size_t)row * row_stride + gate * n + neuron] : 0;
                        wq.push_back(bf16_of_int(v));
                    }
}
}  // namespace

void nnn_model_pack(const RNNModel &m, std::vector<uint16_t> &wq, std::vector<float> &fpar, nnn::RnnPlan &plan, nnn::ModelDims &md)
{
    wq.clear();
    fpar.clear();
    const int nd = m.input_dense.nb_neurons, nv = m.vad_gru.nb_neurons, nn = m.noise_gru.nb_neurons,
              ndn = m.denoise_gru.nb_neurons;
    md.nd = nd; md.nv = nv; md.nn = nn; md.ndn = ndn;
    md.act_d = m.input_dense.activation; md.act_v = m.vad_gru.activation; md.act_n = m.noise_gru.activation;
    md.act_dn = m.denoise_gru.activation; md.act_o = m.denoise_output.activation; md.act_vo = m.vad_output.activation;
    // where everything goes is the plan's to say (nnn_layout.h); here the weights and biases are laid out to it
    plan = nnn::rnn_plan_for(nd, nv, nn, ndn);
    plan.dense.act = md.act_d; plan.vad.act = md.act_v; plan.noise.act = md.act_n; plan.dn.act = md.act_dn; plan.out.act = md.act_o;
    plan.act_vo = md.act_vo;
    const int8_t *blob = m.blob.data();
    const int cV = plan.cV, cF = plan.cF, cD = plan.dense.out_col, NF = 42;
    auto fbias = [&](int at, size_t ofs, int count) {
        assert(fpar.size() == (size_t)at);
        for (int i = 0; i < count; i++) fpar.push_back((float)blob[ofs + i]);
    };
    // input dense: features -> D                                  (ref: src/rnn.rs:353-355)
    pack_gemm(wq, plan.dense.in, blob + m.input_dense.weights, nd, nd, [&](int k) { return (k >= cF && k < cF + NF) ? k - cF : -1; });
    fbias(plan.dense.bias, m.input_dense.bias, nd);
    // vad GRU: input D                                             (ref: src/rnn.rs:356-358)
    pack_gemm(wq, plan.vad.in, blob + m.vad_gru.weights, 3 * nv, nv, [&](int k) { return (k >= cD && k < cD + nd) ? k - cD : -1; });
    pack_gemm(wq, plan.vad.rec, blob + m.vad_gru.rec, 3 * nv, nv, [&](int k) { return k < nv ? k : -1; });
    fbias(plan.vad.bias, m.vad_gru.bias, 3 * nv);
    // noise GRU: reference input order [D | V | F]                 (ref: src/rnn.rs:361-366)
    pack_gemm(wq, plan.noise.in, blob + m.noise_gru.weights, 3 * nn, nn, [&](int k) {
        if (k >= cV && k < cV + nv) return nd + (k - cV);
        if (k >= cF && k < cF + NF) return nd + nv + (k - cF);
        if (k >= cD && k < cD + nd) return k - cD;
        return -1;
    });
    pack_gemm(wq, plan.noise.rec, blob + m.noise_gru.rec, 3 * nn, nn, [&](int k) { return k < nn ? k : -1; });
    fbias(plan.noise.bias, m.noise_gru.bias, 3 * nn);
    // denoise GRU: reference input order [V | N | F]               (ref: src/rnn.rs:368-377)
    pack_gemm(wq, plan.dn.in, blob + m.denoise_gru.weights, 3 * ndn, ndn, [&](int k) {
        if (k < nn) return nv + k;
        if (k >= cV && k < cV + nv) return k - cV;
        if (k >= cF && k < cF + NF) return nv + nn + (k - cF);
        return -1;
    });
    pack_gemm(wq, plan.dn.rec, blob + m.denoise_gru.rec, 3 * ndn, ndn, [&](int k) { return k < ndn ? k : -1; });
    fbias(plan.dn.bias, m.denoise_gru.bias, 3 * ndn);
    // gains: denoise state (written to columns 0..ndn) -> 22       (ref: src/rnn.rs:378)
    pack_gemm(wq, plan.out.in, blob + m.denoise_output.weights, 22, 22, [&](int k) { return k < ndn ? k : -1; });
    fbias(plan.out.bias, m.denoise_output.bias, 22);
    // vad output, 1 x nv, stays on the vector ALU                  (ref: src/rnn.rs:359)
    fbias(plan.vo_w, m.vad_output.weights, nv);
    fbias(plan.vo_b, m.vad_output.bias, 1);
    assert(wq.size() == (size_t)nnn::rnn_plan_wq_len(plan) * 8 && fpar.size() == (size_t)nnn::rnn_plan_fpar_len(plan));
}

// ---- model entry points -------------------------------------------------------------------------
extern "C" RNNModel *nnn_model_from_bytes(const uint8_t *bytes, size_t len)
{
    RNNModel *m = nnn_model_parse(bytes, len);
    if (!m) nnn_set_error("malformed .rnn model");
    return m;
}
extern "C" RNNModel *nnn_model_default(void)
{
    size_t len;
    const uint8_t *w = nnn_builtin_weights(&len);
    return nnn_model_parse(w, len);
}
// RNNoise text model -> .rnn bytes (ref: train/convert_rnnoise.py:18-29).  Python's str.strip / str.split / int():
// ASCII whitespace separators, optional sign, decimal digits (int() also takes '_' separators and non-ASCII digits;
// no model file uses them and they are rejected here).
extern "C" long nnn_convert_rnnoise_text(const char *text, size_t len, uint8_t *out, size_t cap)
{
    static const char kHeader[] = "rnnoise-nu model file version 1";
    auto is_ws = [](char c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
    auto not_an_integer = [](long n) {
        char msg[64];
        snprintf(msg, sizeof(msg), "token %ld is not an integer", n);
        nnn_set_error(msg);
    };
    if (!text) { nnn_set_error("null text"); return -1; }
    size_t eol = 0;
    while (eol < len && text[eol] != '\n') eol++;
    size_t a = 0, b = eol;
    while (a < b && is_ws(text[a])) a++;
    while (b > a && is_ws(text[b - 1])) b--;
    if (b - a != sizeof(kHeader) - 1 || memcmp(text + a, kHeader, b - a) != 0) { nnn_set_error("Unexpected input file format"); return -1; }
    long n = 0;
    size_t i = eol < len ? eol + 1 : len;
    while (i < len) {
        while (i < len && is_ws(text[i])) i++;
        if (i >= len) break;
        bool neg = false;
        if (text[i] == '+' || text[i] == '-') neg = text[i++] == '-';
        if (i >= len || text[i] < '0' || text[i] > '9') { not_an_integer(n); return -1; }
        unsigned v = 0;   // only the value modulo 256 matters
        while (i < len && text[i] >= '0' && text[i] <= '9') v = (v * 10u + (unsigned)(text[i++] - '0')) & 0xffffu;
        if (i < len && !is_ws(text[i])) { not_an_integer(n); return -1; }
        const uint8_t byte = (uint8_t)((neg ? 256u - (v & 255u) : v) & 255u);   // Python's non-negative modulo
        if (out) {
            if ((size_t)n >= cap) { nnn_set_error("output buffer too small"); return -1; }
            out[n] = byte;
        }
        n++;
    }
    return n;
}
extern "C" RNNModel *nnn_model_from_rnnoise_text(const char *text, size_t len)
{
    const long n = nnn_convert_rnnoise_text(text, len, nullptr, 0);
    if (n < 0) return nullptr;
    std::vector<uint8_t> bytes((size_t)n);
    if (nnn_convert_rnnoise_text(text, len, bytes.data(), bytes.size()) != n) return nullptr;
    return nnn_model_from_bytes(bytes.data(), bytes.size());
}
extern "C" void nnn_model_free(RNNModel *m) { delete m; }
// RnnModel is Clone in the reference (#[derive(Clone)], src/rnn.rs:54): an independent copy of the parameters
extern "C" RNNModel *nnn_model_clone(const RNNModel *m)
{
    if (!m) {
        nnn_set_error("null model");
        return nullptr;
    }
    return new RNNModel(*m);
}
extern "C" void nnn_model_shape(const RNNModel *m, int32_t s[12])
{
    s[0] = m->input_dense.nb_inputs; s[1] = m->input_dense.nb_neurons; s[2] = m->vad_gru.nb_neurons;
    s[3] = m->noise_gru.nb_neurons; s[4] = m->denoise_gru.nb_neurons; s[5] = m->denoise_output.nb_neurons;
    s[6] = m->input_dense.activation; s[7] = m->vad_gru.activation; s[8] = m->noise_gru.activation;
    s[9] = m->denoise_gru.activation; s[10] = m->denoise_output.activation; s[11] = m->vad_output.activation;
}

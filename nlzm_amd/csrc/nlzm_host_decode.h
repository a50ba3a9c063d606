// nlzm_host_decode.h -- the host decoder: decode_file (NLZM.cpp:1912-2039) on a byte range.
//
// This is the SPECIFICATION of the stream's bytes for everything in this repository that reads them: the command line
// (nlzm_cli.cpp: `d` / `t`) runs it, and the device decoder role (nlzm_decode.h) is tested against it byte for byte, on
// reference streams and on damaged ones (tests/host_sim/decode_sim.cpp).  Where the two disagree this file is right.
// Host code only; header-only so that the CLI and the test harness include the same text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace nlzm_host {

struct Cdf { uint16_t c[17]; };
struct Model {
    uint32_t rep[4];
    Cdf cmd, lit_hi, lit_lo[16], len_direct, len_ext_hi, len_ext_lo[16], slot_hi[4], slot_lo[4][8];
};
inline void cdf_set(Cdf &d, int ns) { for (int i = 0; i <= ns; i++) d.c[i] = (uint16_t)(i * (16384 / ns)); }
inline void model_init(Model &m)
{
    for (int i = 0; i < 4; i++) m.rep[i] = (uint32_t)i + 1;
    cdf_set(m.cmd, 4); cdf_set(m.lit_hi, 16); cdf_set(m.len_direct, 8); cdf_set(m.len_ext_hi, 16);
    for (int i = 0; i < 16; i++) { cdf_set(m.lit_lo[i], 16); cdf_set(m.len_ext_lo[i], 16); }
    for (int c = 0; c < 4; c++) { cdf_set(m.slot_hi[c], 8); for (int i = 0; i < 8; i++) cdf_set(m.slot_lo[c][i], 8); }
}
inline void cdf_adapt(Cdf &d, int ns, int y)
{
    for (int i = 0; i < ns; i++) {
        const int mix = i <= y ? i : 16384 + i + (127 - ns);                       // :284-298
        d.c[i] = (uint16_t)(d.c[i] + ((mix - (int)d.c[i]) >> 7));                 // :348-382
    }
}
inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// what a decode counted (the oracle's counters of the same names: rans_syms, bit_ops, n_literal, n_dict, n_rep)
struct Counts { uint64_t syms = 0, raw_ops = 0, n_literal = 0, n_dict = 0, n_rep = 0; };

struct Frame {
    const uint8_t *bits, *rans, *end;
    uint32_t word = 0, word_bits = 0, num_ops = 0, st[4], idx = 0;
    bool bad = false;
    Counts *cnt = nullptr;
    int sym(Cdf &d, int nbits)                                                    // ReadCDF, :666-712
    {
        num_ops--;
        if (cnt) cnt->syms++;
        uint32_t &rs = st[idx++ & 3];
        const uint32_t f = rs & 16383u;
        int y = 0;
        for (int step = 1 << (nbits - 1); step; step >>= 1) y += step * (f >= d.c[y + step]);   // :388-433
        const uint32_t start = d.c[y], freq = (uint32_t)d.c[y + 1] - start;
        uint32_t x = freq * (rs >> 14) + f - start;                               // :457-459
        if (x < 65536u) {                                                         // :481-488
            if (rans + 2 > end) { bad = true; return 0; }
            x = (x << 16) + ((uint32_t)rans[0] << 8) + rans[1];
            rans += 2;
        }
        rs = x;
        cdf_adapt(d, 1 << nbits, y);
        return y;
    }
    uint32_t raw(uint32_t nb)                                                     // ReadBits, :714-731
    {
        num_ops--;
        if (cnt) cnt->raw_ops++;
        while (word_bits < 24) {
            if (bits >= end) { bad = true; return 0; }
            word |= (uint32_t)*bits++ << (24 - word_bits);
            word_bits += 8;
        }
        const uint32_t y = word >> (32 - nb);
        word <<= nb; word_bits -= nb;
        return y;
    }
};
inline uint32_t match_min(uint32_t d) { return 2u + (d >= 256u) + (d >= 4096u) + (d >= (1u << 20)); }   // :813-821
inline void rep_add(uint32_t r[4], uint32_t d)
{
    if (r[0] == d || r[1] == d || r[2] == d || r[3] == d) return;
    r[3] = r[2]; r[2] = r[1]; r[1] = r[0]; r[0] = d;
}
inline uint32_t dec_len(Frame &f, Model &m)                                       // model_decode_lv, :1369-1383
{
    uint32_t lv = (uint32_t)f.sym(m.len_direct, 3);
    if (lv == 7) {
        const int hi = f.sym(m.len_ext_hi, 4);
        const int lo = f.sym(m.len_ext_lo[hi], 4);
        lv += ((uint32_t)hi << 4) + (uint32_t)lo;
    }
    return lv;
}

// A byte range of the file as the decoder sees it
struct Span {
    const uint8_t *p; size_t n;
    size_t size() const { return n; }
    const uint8_t &operator[](size_t i) const { return p[i]; }
    const uint8_t *data() const { return p; }
};

// Length of the stream that starts at in[0]: header, frames hopped over by the sizes their headers carry (:645-663),
// terminator (:646-648).  0: malformed.  Block mode (k independent streams back to back) is split with this.
inline size_t stream_length(const Span &in)
{
    if (in.size() < 8) return 0;
    size_t pos = 4;
    for (;;) {
        if (pos + 4 > in.size()) return 0;
        if (!be32(&in[pos])) return pos + 4;
        if (pos + 12 > in.size()) return 0;
        const uint32_t nb = be32(&in[pos + 4]), nr = be32(&in[pos + 8]);
        if (nb < 12 || nr < 16 || pos + (size_t)nb + nr > in.size()) return 0;
        pos += (size_t)nb + nr;
    }
}

// The split of a container by its frame headers: the lengths of the streams that lie back to back from in[0], at most `max` of them,
// up to the first bytes that are no stream.  Returns how many there are.
inline size_t split_streams(const Span &in, size_t max, std::vector<uint64_t> &len)
{
    len.clear();
    for (size_t pos = 0; len.size() < max && pos < in.size();) {
        const size_t l = stream_length(Span{ in.p + pos, in.size() - pos });
        if (!l) break;
        len.push_back(l);
        pos += l;
    }
    return len.size();
}

// (distance, length) of every match, for tests that must know what a stream contains
struct MatchLog { std::vector<uint32_t> dv, lv; std::vector<uint64_t> at; };      // at: the output offset a match starts at

// returns 0 or a negative code; out receives the decoded bytes
inline int decode_stream(const Span &in, std::vector<uint8_t> &out, uint32_t *hist_bits, uint32_t *frame_bits, Counts *cnt = nullptr,
                         MatchLog *log = nullptr)
{
    if (in.size() < 8) return -1;
    const uint32_t hb = ((uint32_t)in[0] << 8) + in[1], fb = ((uint32_t)in[2] << 8) + in[3];
    *hist_bits = hb; *frame_bits = fb;
    // the reference asserts 12 <= hist_bits (:1918) although its encoder can write 10 or 11 for
    // inputs under 2 KiB (:1716); this decoder accepts those streams too
    if (hb < 10 || hb > 28 || fb < 12 || fb > 20) return -2;
    Model *m = new Model;
    model_init(*m);
    size_t pos = 4;
    int rc = 0;
    for (;;) {
        if (pos + 4 > in.size()) { rc = -3; break; }
        Frame f;
        f.cnt = cnt;
        f.num_ops = be32(&in[pos]);
        if (!f.num_ops) break;
        if (pos + 12 > in.size()) { rc = -3; break; }
        const uint32_t nb = be32(&in[pos + 4]), nr = be32(&in[pos + 8]);
        if (nb < 12 || nr < 16 || pos + (size_t)nb + nr > in.size()) { rc = -3; break; }
        f.bits = &in[pos + 12]; f.rans = &in[pos + nb]; f.end = in.data() + pos + nb + nr;
        for (int i = 0; i < 4; i++) { f.st[i] = f.rans[0] | (f.rans[1] << 8) | (f.rans[2] << 16) | ((uint32_t)f.rans[3] << 24); f.rans += 4; }
        while (f.num_ops > 0 && !f.bad) {
            const int cmd = f.sym(m->cmd, 2);
            if (cmd == 0) {
                const int hi = f.sym(m->lit_hi, 4);
                const int lo = f.sym(m->lit_lo[hi], 4);
                out.push_back((uint8_t)((hi << 4) + lo));
                if (cnt) cnt->n_literal++;
                continue;
            }
            uint32_t lv, dv;
            if (cmd == 1) {
                lv = dec_len(f, *m);
                const uint32_t lc = lv < 3 ? lv : 3;
                const int shi = f.sym(m->slot_hi[lc], 3);
                const int slo = f.sym(m->slot_lo[lc][shi], 3);
                dv = ((uint32_t)shi << 3) + (uint32_t)slo;
                if (dv >= 4) {                                                    // :1395-1413
                    uint32_t ab = (dv >> 1) - 1;
                    dv = (2 + (dv & 1)) << ab;
                    if (ab < 4) dv += f.raw(ab);
                    else { ab -= 4; if (ab > 0) dv += f.raw(ab) << 4; dv += f.raw(4); }
                }
                dv += 1;
                if (cnt) cnt->n_dict++;
            } else if (cmd == 2) {
                const uint32_t ri = f.raw(2);
                lv = dec_len(f, *m);
                dv = m->rep[ri];
                if (cnt) cnt->n_rep++;
            } else { rc = -5; break; }
            lv += match_min(dv);
            rep_add(m->rep, dv);
            if (dv > out.size()) { rc = -6; break; }
            if (log) { log->dv.push_back(dv); log->lv.push_back(lv); log->at.push_back(out.size()); }
            const size_t from = out.size() - dv;
            for (uint32_t i = 0; i < lv; i++) out.push_back(out[from + i]);
        }
        if (rc) break;
        if (f.bad) { rc = -7; break; }
        pos += (size_t)nb + nr;
    }
    delete m;
    return rc;
}

}  // namespace nlzm_host

// nlzm_cli.cpp -- host side of the MI355X build: NLZM's own command line
// (NLZM.cpp:2050-2178) in one file.  `c` runs the compress path on the GPU through
// the C ABI of include/nlzm_hip.h and fails if no gfx950 device is present;
// `d`/`t` decode on the host (the decoder is a serial byte-copy machine and stays
// on the CPU: SURVEY.md 8f-1); `h` prints the CRC32; `x` (not in the reference) writes byte ranges of what
// a block container holds, reading only the blocks they need (host decoder, or nlzm_hip_read_ranges with -gpu).
// main() reads the flags and hands over to one function per command; the sidecar index is nlzm_index.h's.
//
// Messages, flag handling and exit codes follow the reference:
//   flags lower-cased, leading '-' stripped, -window:N clamped to [15,28]   :2074-2092
//   "Error: %s already exists" / "Error: %s file does not exist", return -1   :2095-2112
//   banner and usage text                                                     :2051, :2165-2171
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <exception>
#include <memory>
#include <thread>
#include <string>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_host_decode.h"
#include "nlzm_read_plan.h"
#include "nlzm_container_plan.h"       // (kMaxBlocks)
#include "nlzm_index.h"

namespace {

// ---- CRC32 (crc32_calc, NLZM.cpp:126-199; display only, never stored) ---------
uint32_t crc_table[256];
void crc_init()
{
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        crc_table[n] = c;
    }
}
uint32_t crc_calc(const uint8_t *p, uint64_t n, uint32_t crc)
{
    uint32_t c = crc ^ 0xFFFFFFFFu;
    while (n--) c = crc_table[(c ^ *p++) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

bool slurp(const char *path, std::vector<uint8_t> &buf)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseeko(f, 0, SEEK_END);
    const long long sz = ftello(f);
    fseeko(f, 0, SEEK_SET);
    buf.resize((size_t)sz);
    const bool ok = !sz || fread(buf.data(), 1, (size_t)sz, f) == (size_t)sz;
    fclose(f);
    return ok;
}
bool refuse_existing(const char *path)
{
    FILE *probe = fopen(path, "rb");
    if (probe) { printf("Error: %s already exists\n", path); fclose(probe); }
    return probe != nullptr;
}
int hip_error(const char *what = "") { printf("Error: %s%s\n", what, nlzm_hip_last_error()); return -1; }
double seconds(const timespec &a, const timespec &b) { return (double)(b.tv_sec - a.tv_sec) + 1e-9 * (double)(b.tv_nsec - a.tv_nsec); }

// The output file of c and d.  Whatever way the command ends, the file is removed again unless done() said that it stays.
struct OutFile {
    const char *path = nullptr;
    FILE *f = nullptr;
    bool open(const char *p) { path = p; f = fopen(p, "wb"); return f != nullptr; }
    void done() { if (f) fclose(f); f = nullptr; }
    ~OutFile() { if (f) { fclose(f); remove(path); } }
};

// one host thread per block, all of them joined
template <class Fn>
void for_each_block(size_t k, Fn fn)
{
    std::vector<std::thread> th;
    for (size_t i = 0; i < k; i++) th.emplace_back([&fn, i] { fn(i); });
    for (auto &t : th) t.join();
}

// digits and nothing else; a number over `max` is refused, not saturated
bool parse_uint(const char *&p, unsigned long long max, unsigned long long &v)
{
    if (*p < '0' || *p > '9') return false;
    for (v = 0; *p >= '0' && *p <= '9'; p++) {
        const unsigned long long d = (unsigned long long)(*p - '0');
        if (v > (max - d) / 10) return false;
        v = v * 10 + d;
    }
    return true;
}

// ---- host decoder: decode_file (NLZM.cpp:1912-2039), shared with the device decoder's test harness ----------
using nlzm_host::Span;
using nlzm_host::stream_length;
using nlzm_host::decode_stream;
using nlzm::index::Index;

void lower(char *v) { for (; *v; v++) *v = (char)(*v | 0x20); }

// ---- -elem:E: the byte planes of a typed block undone on the host (the rule of nlzm_planes.h restated: y[j m + i] = x[i e + j], the tail as it is) ----
void planes_undo(const uint8_t *y, uint8_t *x, uint64_t n, uint32_t e)
{
    const uint64_t m = n / e;
    for (uint32_t j = 0; j < e; j++) for (uint64_t i = 0; i < m; i++) x[i * e + j] = y[j * m + i];
    for (uint64_t t = e * m; t < n; t++) x[t] = y[t];
}

struct ByteRange { uint64_t off, len; };
struct Options {
    uint32_t hist_bits = 22;                        // :2071
    uint32_t nblocks = 1;                           // -blocks:k (not in the reference): k independent streams, back to back
    uint32_t ngpus = 0;                             // -gpus:g (not in the reference): the blocks on g GPUs of this node, -blocks:k on each
    bool verify = false;                            // -verify (not in the reference): c decodes what it wrote on the device and compares it with the input
    bool with_crc = false;                          // -crc (not in the reference): c keeps every block's CRC32, hashed on the device, in the index (NLZMIDX 2); d / t check them
    bool on_gpu = false;                            // -gpu (not in the reference): d / t decode on the device; without it they are host-only and need none
    uint32_t cdc_bits = 0;                          // -cdc:B (not in the reference): c cuts the blocks by content on the device, 2^B bytes a block on average
    bool dedup = false;                             // -dedup (not in the reference): with -cdc:B, c does not compress a block again whose bytes an earlier block holds
    uint32_t elem = 0;                              // -elem:E (not in the reference): c compresses every block's byte planes at element size E (NLZMIDX 3); d / t undo them
    uint32_t steps_k = 0;                           // -steps:K (not in the reference): d -gpu / t -gpu decode in steps of K frames per block
    std::vector<ByteRange> ranges;                  // -range:off:len (not in the reference): what x writes, in this order
};

// What each reader takes of an index.  d / t: every version, fields behind the last block let pass, 4096 blocks (c -blocks:k writes up to 65,536:
// DESIGN.md section 17).  x: versions 1 and 2 -- it does not read typed blocks --, 65,536 blocks, nothing behind the last block.
const nlzm::index::Accept kDecodeTakes{ 3, 4096, true }, kExtractTakes{ 2, nlzm::container::kMaxBlocks, false };

// ---- c ---------------------------------------------------------------------------------------------------------------------------------
// the reference's summary (:1755-1759): sizes of its own structures for this window
void print_summary(uint64_t in_size, uint32_t hist_bits, uint32_t nstreams)
{
    uint32_t hb, fb, cs, feed;
    nlzm_hip_geometry(in_size, hist_bits, &hb, &fb, &cs, &feed);
    const uint32_t c1 = hb < 15 ? 15 : (hb > 17 ? 17 : hb), c2 = hb < 16 ? 16 : (hb > 20 ? 20 : hb), c3 = hb < 16 ? 16 : (hb > 22 ? 22 : hb);
    const uint64_t mf = (4ull << 12) + (8ull << (12 + c1 - 15)) + (4ull << (13 + c2 - 16)) + (8ull << hb) + (4ull << (15 + c3 - 16));
    printf("Model: %d KB\n", 2);
    printf("Parser: %d KB\n", 65);
    printf("Dictionary: %d KB\n", (int)(((1ull << hb) + 1023) >> 10));
    printf("Frame: %d KB\n", (int)(((1u << fb) + 1023) >> 10));
    printf("Dictionary search: %d KB\n", (int)((mf + 1023) >> 10));
    if (nstreams > 1)
        printf("Note: %u independent streams are written back to back; this program's d/t read them, the reference's d "
               "stops after the first\n", nstreams);
    printf("Working...\r");
}

// The block index, a sidecar: where every block's stream starts, how long it is and how many input bytes it holds.  The
// streams stay self-delimiting -- the index only saves d/t the hop over every frame header of every block before the parallel decode can
// start, and keeps the later blocks' boundaries when the container is damaged inside an earlier one.
void write_index(const char *out_path, const Index &ix)
{
    const std::string ip = std::string(out_path) + ".idx";
    if (FILE *fi = fopen(ip.c_str(), "wb")) {
        nlzm::index::write(fi, ix);
        fclose(fi);
        printf("Block index: %s\n", ip.c_str());
    }
}

// read, uploaded and compressed piece by piece (nlzm_hip_feed_*): the file is never whole in host memory
int compress_one_stream(const Options &o, const char *in_path, const char *out_path)
{
    FILE *fin = fopen(in_path, "rb");
    if (!fin) { printf("Error: %s file does not exist\n", in_path); return -1; }
    fseeko(fin, 0, SEEK_END);
    const uint64_t in_size = (uint64_t)ftello(fin);
    fseeko(fin, 0, SEEK_SET);
    OutFile fout;
    if (!fout.open(out_path)) { printf("Error: %s file does not exist\n", out_path); fclose(fin); return -1; }
    if (nlzm_hip_init(0)) return hip_error();
    print_summary(in_size, o.hist_bits, 1);
    uint64_t out_n = 0;
    struct timespec w0, w1;
    clock_gettime(CLOCK_MONOTONIC, &w0);
    // the reference's loop in big steps: read a piece, hand it over, write the frames that are finished (:1774-1778, :1853, :1870-1885)
    std::vector<uint8_t> piece(16u << 20), obuf(16u << 20);
    uint32_t crc = 0;
    int rc = nlzm_hip_feed_begin(in_size, o.hist_bits);
    auto drain = [&]() {
        for (uint64_t got = 1; !rc && got;) {
            rc = nlzm_hip_feed_output(obuf.data(), obuf.size(), &got);
            if (!rc && got) { fwrite(obuf.data(), 1, (size_t)got, fout.f); out_n += got; }
        }
    };
    for (uint64_t done = 0; !rc && done < in_size;) {
        const size_t m = (size_t)(in_size - done < piece.size() ? in_size - done : piece.size());
        if (fread(piece.data(), 1, m, fin) != m) { printf("Error: %s could not be read\n", in_path); rc = -1; break; }
        if (!o.with_crc) crc = crc_calc(piece.data(), m, crc);
        rc = nlzm_hip_feed(piece.data(), m);
        done += m;
        drain();
        printf("Working... %" PRIu64 " -> %" PRIu64 "\r", done, out_n);
        fflush(stdout);
    }
    if (!rc) rc = nlzm_hip_feed_finish();
    drain();
    if (!rc && o.with_crc) rc = nlzm_hip_feed_input_crc32(&crc);      // (the input is whole in HBM and nowhere on the host: hashed where it lies)
    nlzm_hip_feed_end();
    fclose(fin);
    clock_gettime(CLOCK_MONOTONIC, &w1);
    if (rc) return rc != -1 ? hip_error() : -1;
    fout.done();
    if (o.with_crc) {
        Index ix;
        ix.version = 2; ix.n_in = in_size; ix.n_out = out_n; ix.whole = crc;
        ix.off = { 0 }; ix.len = { out_n }; ix.raw = { in_size }; ix.crc = { crc };
        write_index(out_path, ix);
    }
    printf("Working... %" PRIu64 " -> %" PRIu64 "\n", in_size, out_n);
    printf("Done (input CRC32 %X, %.2f sec)\n", crc, seconds(w0, w1));
    nlzm_hip_shutdown();
    return 0;
}

// every block's bytes of the input: cut by content on the device (-cdc:B), or the equal partition; with -elem:E, whole elements a block
bool partition(const Options &o, const std::vector<uint8_t> &in, std::vector<uint64_t> &boff, std::vector<uint64_t> &braw)
{
    if (!o.cdc_bits) {
        const uint32_t nstreams = o.ngpus ? o.ngpus * o.nblocks : o.nblocks;
        uint64_t per = (in.size() + nstreams - 1) / nstreams;
        if (o.elem) per = (per + o.elem - 1) / o.elem * o.elem;
        for (uint32_t i = 0; i < nstreams; i++) {
            const uint64_t lo = (uint64_t)i * per < in.size() ? (uint64_t)i * per : in.size(), hi = lo + per < in.size() ? lo + per : in.size();
            boff.push_back(lo); braw.push_back(hi - lo);
        }
        return true;
    }
    // the cut points from the device, with the default lengths: 2^(B - 2) .. 2^(B + 2) bytes a block (2^31 at most)
    const uint64_t min_len = 1ull << (o.cdc_bits - 2), max_len = o.cdc_bits + 2 > 31 ? 1ull << 31 : 1ull << (o.cdc_bits + 2);
    std::vector<uint64_t> cuts(nlzm::container::kMaxBlocks - 1);
    uint32_t ncuts = 0;
    const int rc = nlzm_hip_cut_points(in.data(), in.size(), o.cdc_bits, min_len, max_len, cuts.data(), (uint32_t)cuts.size(), &ncuts);
    if (rc == NLZM_HIP_E_CAPACITY) printf("Error: -cdc:%u cuts this input into %" PRIu64 " blocks, a container holds %u at most: raise B\n", o.cdc_bits, (uint64_t)ncuts + 1, nlzm::container::kMaxBlocks);
    else if (rc) hip_error();
    if (rc) return false;
    if (o.elem) {                                   // (the cuts rounded down, equal ones dropped)
        uint32_t kept = 0;
        for (uint32_t i = 0; i < ncuts; i++) {
            const uint64_t c = cuts[i] / o.elem * o.elem;
            if (c && (!kept || c > cuts[kept - 1])) cuts[kept++] = c;
        }
        ncuts = kept;
    }
    for (uint32_t i = 0; i <= ncuts; i++) {
        const uint64_t lo = i ? cuts[i - 1] : 0, hi = i < ncuts ? cuts[i] : (uint64_t)in.size();
        boff.push_back(lo); braw.push_back(hi - lo);
    }
    printf("Blocks: %u (cut by content)\n", ncuts + 1);
    return true;
}

// the input whole, one call: blocks, -verify, -crc, the index (-verify, -cdc and -elem need the input whole, so one stream with them comes here too)
int compress_container(const Options &o, const char *in_path, const char *out_path)
{
    const uint32_t ngpus = o.ngpus, nblocks = o.nblocks, elem = o.elem;
    std::vector<uint8_t> in;
    if (!slurp(in_path, in)) { printf("Error: %s file does not exist\n", in_path); return -1; }
    OutFile fout;
    if (!fout.open(out_path)) { printf("Error: %s file does not exist\n", out_path); return -1; }
    if (!ngpus && nlzm_hip_init(0)) return hip_error();
    std::vector<uint64_t> boff, braw;
    if (!partition(o, in, boff, braw)) return -1;
    const uint32_t nstreams = (uint32_t)boff.size();
    print_summary(in.size(), o.hist_bits, nstreams);
    uint64_t out_n = 0;
    struct timespec w0, w1;
    clock_gettime(CLOCK_MONOTONIC, &w0);
    // room for the streams (a guaranteed bound: 9.7 GB at 65,536 blocks).  Not a vector: nothing is filled, and the pages behind the streams' end are never touched
    const size_t out_room = ngpus ? (size_t)nlzm_hip_compress_bound(in.size()) + (size_t)nstreams * (16 + 131072)
                          : o.cdc_bits || elem ? (size_t)nlzm_hip_compress_ranges_bound(nstreams, braw.data()) : (size_t)nlzm_hip_compress_blocks_bound(in.size(), nblocks);
    struct Room { uint8_t *p; size_t n; uint8_t *data() const { return p; } size_t size() const { return n; } ~Room() { free(p); } } out{ (uint8_t *)malloc(out_room ? out_room : 1), out_room };
    if (!out.data()) { printf("Error: no memory for %zu bytes of output\n", out_room); return -1; }
    std::vector<uint64_t> blen(nstreams);
    std::vector<int> devs;
    for (uint32_t d = 0; d < ngpus; d++) devs.push_back((int)d);
    if (o.dedup && nlzm_hip_set_option("dedup_ranges", 1)) return hip_error();
    const std::vector<uint8_t> elems(nstreams, (uint8_t)elem);
    const int rc = elem ? nlzm_hip_compress_ranges_typed(in.data(), in.size(), nstreams, boff.data(), braw.data(), elems.data(), o.hist_bits, out.data(), out.size(), blen.data(), &out_n)
                 : o.cdc_bits ? nlzm_hip_compress_ranges(in.data(), in.size(), nstreams, boff.data(), braw.data(), o.hist_bits, out.data(), out.size(), blen.data(), &out_n)
                 : ngpus ? nlzm_hip_compress_blocks_multi(devs.data(), ngpus, nblocks, in.data(), in.size(), o.hist_bits, out.data(), out.size(), blen.data(), &out_n)
                 : nblocks > 1 ? nlzm_hip_compress_blocks(in.data(), in.size(), nblocks, o.hist_bits, out.data(), out.size(), blen.data(), &out_n)
                               : nlzm_hip_compress(in.data(), in.size(), o.hist_bits, out.data(), out.size(), &out_n);
    clock_gettime(CLOCK_MONOTONIC, &w1);
    if (rc) return hip_error();
    if (nstreams == 1) blen[0] = out_n;
    if (o.dedup) {          // (the finder's counters of the call: the blocks that were another's copy, and their bytes)
        uint64_t distinct = nstreams, dup_bytes = 0;
        (void)nlzm_hip_get_counter("dedup_distinct", &distinct);
        (void)nlzm_hip_get_counter("dedup_dup_bytes", &dup_bytes);
        printf("Duplicates: %" PRIu64 " of %u blocks (%" PRIu64 " bytes) not compressed again\n", (uint64_t)nstreams - distinct, nstreams, dup_bytes);
    }
    if (o.verify) {
        // the stream(s) decoded on the device, one workgroup each, and compared there with the input; neither comes back to the host
        uint64_t first = 0, decoded = 0;
        struct timespec v0, v1;
        clock_gettime(CLOCK_MONOTONIC, &v0);
        int vrc = ngpus ? nlzm_hip_init(0) : 0;
        if (!vrc && elem) {
            // typed blocks: decoded through the typed entry point, which undoes the planes, and compared here (the blocks are the input, in order)
            std::vector<uint8_t> back(in.size());
            vrc = nlzm_hip_decompress_blocks_typed(out.data(), out_n, nstreams, blen.data(), braw.data(), elems.data(), back.data(), back.size(), nullptr, &decoded);
            for (first = 0; !vrc && first < decoded && first < in.size() && back[first] == in[first];) first++;
        } else
        if (!vrc) vrc = nlzm_hip_verify(out.data(), out_n, nstreams, nstreams > 1 ? blen.data() : nullptr, in.data(), in.size(), &first, &decoded);
        clock_gettime(CLOCK_MONOTONIC, &v1);
        if (vrc) return hip_error("verify: ");
        if (!NLZM_HIP_VERIFY_EQUAL(first, decoded, (uint64_t)in.size())) {
            if (first < in.size() && first < decoded) printf("Verify FAILED: the stream decodes to something else from offset %" PRIu64 "; %s removed\n", first, out_path);
            else printf("Verify FAILED: the stream decodes to %" PRIu64 " bytes, the input has %" PRIu64 " (equal up to offset %" PRIu64 "); %s removed\n", decoded, (uint64_t)in.size(), first, out_path);
            return -3;
        }
        uint64_t dev_us = 0;
        (void)nlzm_hip_get_counter("decode_us", &dev_us);
        printf("Verified (%.2f sec, %.2f of them decoding on the device)\n", seconds(v0, v1), 1e-6 * (double)dev_us);
    }
    // -crc: every block's CRC32 from the device, on a re-upload of the input as -verify makes one; the whole file's is their combination
    std::vector<uint32_t> bcrc(nstreams, 0);
    uint32_t whole = 0;
    if (o.with_crc) {
        int crc_rc = ngpus ? nlzm_hip_init(0) : 0;
        if (!crc_rc) crc_rc = nlzm_hip_crc32_ranges(in.data(), in.size(), nstreams, boff.data(), braw.data(), bcrc.data());
        if (crc_rc) return hip_error("crc: ");
        for (uint32_t i = 0; i < nstreams; i++) whole = nlzm_hip_crc32_combine(whole, bcrc[i], braw[i]);
    }
    fwrite(out.data(), 1, (size_t)out_n, fout.f);
    fout.done();
    if (nstreams > 1 || o.with_crc || o.cdc_bits || elem) {
        Index ix;                                   // (each block's raw length its true one: the equal partition's, or the content's)
        ix.version = elem ? 3 : o.with_crc ? 2 : 1; ix.n_in = in.size(); ix.n_out = out_n; ix.whole = whole;
        ix.off.assign(nstreams, 0); ix.len = blen; ix.raw = braw; ix.crc = bcrc; ix.elem = elems;
        for (uint32_t i = 1; i < nstreams; i++) ix.off[i] = ix.off[i - 1] + blen[i - 1];
        write_index(out_path, ix);
    }
    printf("Working... %" PRIu64 " -> %" PRIu64 "\n", (uint64_t)in.size(), out_n);
    printf("Done (input CRC32 %X, %.2f sec)\n", o.with_crc ? whole : crc_calc(in.data(), in.size(), 0), seconds(w0, w1));
    nlzm_hip_shutdown();
    return 0;
}

// ---- d / t -----------------------------------------------------------------------------------------------------------------------------
// The streams of what d / t read -- one (the reference's format), or several back to back (block mode) -- and what the index says of them.
struct Found {
    std::vector<Span> parts;
    std::vector<uint64_t> blen;                     // their lengths
    bool by_index = false;                          // the boundaries are the index's; otherwise found by hopping over the frames
    Index ix;                                       // (by index) the index: the parts are its first entries -- all of them, unless the container is cut off
    size_t cut_tail = 0;                            // the container is cut off inside the block behind the last of `parts`: so many bytes of it are there
    uint64_t src_len() const { return (uint64_t)(parts.back().p + parts.back().n - parts[0].p); }
};

Found find_parts(const std::vector<uint8_t> &in, const Index *ix, const char *in_path)
{
    Found f;
    // the sidecar index of a block container, if it is there and fits the file: the blocks' boundaries without hopping over their frames
    if (ix && ix->present) {
        const size_t n = nlzm::index::fits_file(*ix, kDecodeTakes, in.data(), in.size(), f.cut_tail);
        for (size_t i = 0; i < n; i++) f.parts.push_back(Span{ in.data() + ix->off[i], (size_t)ix->len[i] });
        if (n) { f.by_index = true; f.ix = *ix; }
        else printf("Note: %s.idx does not fit this file; the blocks are found by their frame headers\n", in_path);
    }
    for (size_t pos = 0; !f.by_index && pos < in.size();) {
        const Span rest{ in.data() + pos, in.size() - pos };
        const size_t len = stream_length(rest);
        if (!len) {
            // what follows is not a stream: the reference stops at the first terminator (:646-648) and so do we;
            // a container that is cut off inside its first stream is malformed
            if (f.parts.empty()) break;
            // a further stream header (:1915-1921: hist_bits, frame_bits, both big-endian 16-bit) with a frame that is cut off:
            // the complete streams are decoded and written, and the exit status says that the container was cut
            const bool header = rest.n >= 4 && rest.p[0] == 0 && rest.p[1] >= 10 && rest.p[1] <= 28 && rest.p[2] == 0 && rest.p[3] >= 12 && rest.p[3] <= 20;
            if (header) f.cut_tail = rest.n;
            else printf("Note: %zu bytes after the last stream ignored\n", rest.n);
            break;
        }
        f.parts.push_back(Span{ rest.p, len });
        pos += len;
    }
    for (const Span &s : f.parts) f.blen.push_back(s.n);
    return f;
}

// What one way of decoding made of the parts.  failed: an error that is no verdict on the streams, already printed; d / t end with -1.
struct Decoded {
    bool failed = false;
    int rc = 0;                                     // the streams are malformed
    bool index_wrong = false;                       // a block did not decode to the bytes its index entry says it holds
    std::vector<uint8_t> out;
    std::vector<uint32_t> got_crcs;                 // what the blocks decoded to hash to, where the decode hashed them
    uint64_t out_size = 0;
    bool out_on_device = false;                     // nothing of the output is on the host: out_size and got_crcs say what it was
    uint32_t hb = 0, fb = 0;
};
// a device call's answer: a malformed stream is the streams' fault, anything else an error
void device_verdict(Decoded &r, int drc, const Found &f)
{
    if (drc == NLZM_HIP_E_FORMAT) r.rc = -7;
    else if (drc) { hip_error(); r.failed = true; }
    r.hb = f.parts[0].p[1]; r.fb = f.parts[0].p[3];
}

// -gpu -steps:K: the decode in steps of K frames per block (nlzm_hip_decode_*): after every step each block's new bytes are fetched, hashed and --
// d -- written at the block's offset, so the host holds one step's output at a time
Decoded decode_in_steps(Found &f, uint32_t steps_k, FILE *fout)
{
    Decoded r;
    const uint32_t k = (uint32_t)f.parts.size();
    std::vector<uint64_t> raw(k), at(k, 0), done(k, 0), had(k, 0);
    const uint64_t src_len = f.src_len();
    uint64_t total = 0, launches = 0;
    int drc = 0;
    if (f.by_index) raw = f.ix.raw;
    else drc = nlzm_hip_decompress_blocks(f.parts[0].p, src_len, k, f.blen.data(), nullptr, nullptr, 0, raw.data(), &total);      // (no lengths anywhere in the format: a size pass)
    for (uint32_t i = 1; i < k; i++) at[i] = at[i - 1] + raw[i - 1];
    if (!drc) drc = nlzm_hip_decode_begin(f.parts[0].p, src_len, k, f.blen.data(), raw.data(), 0);
    std::vector<uint32_t> crcs(k, 0);
    std::vector<uint8_t> piece;
    int finished = 0;
    bool open = !drc;
    while (!drc && !finished) {
        drc = nlzm_hip_decode_step(steps_k, nullptr, done.data(), &finished, nullptr);
        if (drc) { open = false; break; }           // (a failing step has closed the set)
        for (uint32_t i = 0; i < k && !drc; i++) {
            const uint64_t n = done[i] - had[i];
            if (!n) continue;
            piece.resize((size_t)n);
            drc = nlzm_hip_decode_fetch(at[i] + had[i], n, piece.data());
            if (drc) break;
            crcs[i] = crc_calc(piece.data(), n, crcs[i]);
            if (fout) { fseeko(fout, (off_t)(at[i] + had[i]), SEEK_SET); fwrite(piece.data(), 1, (size_t)n, fout); }
            had[i] = done[i];
        }
    }
    if (!drc) { (void)nlzm_hip_get_counter("decode_steps", &launches); drc = nlzm_hip_decode_finish(nullptr, &total); open = false; }
    if (open) nlzm_hip_decode_abandon();
    if (f.by_index && (drc == NLZM_HIP_E_CAPACITY || drc == NLZM_HIP_E_FORMAT || drc == NLZM_HIP_E_NOMEM)) { r.index_wrong = true; drc = 0; }
    device_verdict(r, drc, f);
    if (r.failed) return r;
    // (a decode that did not come to its end leaves nothing of what its steps wrote: the one-call path writes nothing then either)
    if ((r.index_wrong || r.rc) && fout) { fflush(fout); if (ftruncate(fileno(fout), 0)) {} fseeko(fout, 0, SEEK_SET); }
    if (!r.index_wrong && !r.rc) {
        if (k > 1) printf("Blocks: %d\n", (int)k);
        printf("Steps: %u frames, %" PRIu64 " launches\n", steps_k, launches);
        if (fout) { fflush(fout); if (ftruncate(fileno(fout), (off_t)total)) {} fseeko(fout, 0, SEEK_END); }
        f.ix.raw = raw; r.got_crcs = crcs; r.out_size = total; r.out_on_device = true;        // (the output's CRC32 is the blocks' combined)
    }
    return r;
}

// t -gpu by an index with CRC32s (nlzm_hip_check): decoded into a buffer on the device, every block bounded by its index entry, and hashed there
Decoded check_on_device(const Found &f)
{
    Decoded r;
    const uint32_t k = (uint32_t)f.parts.size();
    std::vector<uint64_t> raw(k);
    uint32_t first_bad = k;
    r.got_crcs.assign(k, 0);
    int drc = nlzm_hip_check(f.parts[0].p, f.src_len(), k, f.blen.data(), f.ix.raw.data(), f.ix.crc.data(), &first_bad, r.got_crcs.data());
    if (!drc && first_bad < k) {
        // a wrong length or a wrong CRC?  The blocks' own lengths say (a size pass; only a container that fails pays for it)
        uint64_t total = 0;
        drc = nlzm_hip_decompress_blocks(f.parts[0].p, f.src_len(), k, f.blen.data(), nullptr, nullptr, 0, raw.data(), &total);
        for (uint32_t i = 0; !drc && i < k; i++) if (raw[i] != f.ix.raw[i]) r.index_wrong = true;
    }
    if (drc == NLZM_HIP_E_NOMEM) { r.index_wrong = true; drc = 0; }
    device_verdict(r, drc, f);
    if (r.failed) return r;
    for (uint32_t i = 0; i < k; i++) r.out_size += f.ix.raw[i];
    r.out_on_device = true;
    if (!r.index_wrong && !r.rc && k > 1) printf("Blocks: %d\n", (int)k);
    if (r.index_wrong || r.rc) { r.out_size = 0; r.got_crcs.clear(); }
    return r;
}

// -gpu: all blocks at once on the device, one workgroup each; boundaries from the parts, raw lengths from the index where it gave them
Decoded decode_on_device(const Found &f)
{
    Decoded r;
    const uint32_t k = (uint32_t)f.parts.size();
    std::vector<uint64_t> raw(k);
    const uint64_t src_len = f.src_len();
    uint64_t total = 0;
    int drc = 0;
    if (f.by_index) {
        // the index says what every block holds: one decode pass, every block bounded by its entry -- a block that decodes to more
        // (NLZM_HIP_E_CAPACITY) or to less (NLZM_HIP_E_FORMAT) than that shows the index to be wrong, and the frame headers decide
        // (the sizes are the index's word and nothing else yet: an index that asks for more memory than the host or the device has is a
        //  wrong index, not a reason to die)
        for (uint32_t i = 0; i < k; i++) total += f.ix.raw[i];
        bool room = true;
        try { r.out.resize((size_t)total); } catch (const std::exception &) { room = false; }
        if (room && f.ix.typed()) drc = nlzm_hip_decompress_blocks_typed(f.parts[0].p, src_len, k, f.blen.data(), f.ix.raw.data(), f.ix.elem.data(), r.out.data(), total, raw.data(), &total);
        else if (room) drc = nlzm_hip_decompress_blocks(f.parts[0].p, src_len, k, f.blen.data(), f.ix.raw.data(), r.out.data(), total, raw.data(), &total);
        if (!room || drc == NLZM_HIP_E_CAPACITY || drc == NLZM_HIP_E_FORMAT || drc == NLZM_HIP_E_NOMEM) { r.index_wrong = true; drc = 0; std::vector<uint8_t>().swap(r.out); }
    } else {
        // no lengths anywhere in the format: a size pass, then the decode
        drc = nlzm_hip_decompress_blocks(f.parts[0].p, src_len, k, f.blen.data(), nullptr, nullptr, 0, raw.data(), &total);
        if (!drc) {
            r.out.resize((size_t)total);
            drc = nlzm_hip_decompress_blocks(f.parts[0].p, src_len, k, f.blen.data(), raw.data(), r.out.data(), total, nullptr, &total);
        }
    }
    device_verdict(r, drc, f);
    if (!r.failed && k > 1) printf("Blocks: %d\n", (int)k);
    return r;
}

// without -gpu: a host thread per stream, the outputs in order; typed blocks' planes undone block by block, by the rule restated above
Decoded decode_on_host(const Found &f)
{
    Decoded r;
    const size_t k = f.parts.size();
    std::vector<std::vector<uint8_t>> outs(k);
    std::vector<int> rcs(k, 0);
    std::vector<uint32_t> hbs(k, 0), fbs(k, 0);
    if (f.ix.has_crc()) r.got_crcs.assign(k, 0);
    for_each_block(k, [&](size_t i) {
        rcs[i] = decode_stream(f.parts[i], outs[i], &hbs[i], &fbs[i]);
        if (!rcs[i] && f.ix.has_crc()) r.got_crcs[i] = crc_calc(outs[i].data(), outs[i].size(), 0);
    });
    for (size_t i = 0; i < k && !r.rc; i++) {
        r.rc = rcs[i];
        if (!r.rc && f.by_index && outs[i].size() != f.ix.raw[i]) r.index_wrong = true;
        if (k == 1) r.out.swap(outs[0]);            // (one stream, the reference's format: no copy of it)
        else r.out.insert(r.out.end(), outs[i].begin(), outs[i].end());
    }
    r.hb = hbs[0]; r.fb = fbs[0];
    if (k > 1 && !r.index_wrong) printf("Blocks: %d\n", (int)k);
    if (f.ix.typed() && !r.rc && !r.index_wrong) {
        std::vector<uint8_t> raw_bytes(r.out.size());
        std::vector<uint64_t> at(k, 0);
        for (size_t i = 1; i < k; i++) at[i] = at[i - 1] + f.ix.raw[i - 1];
        for_each_block(k, [&](size_t i) { planes_undo(r.out.data() + at[i], raw_bytes.data() + at[i], f.ix.raw[i], f.ix.elem[i]); });
        r.out.swap(raw_bytes);
        r.got_crcs.clear();                         // (the CRC32s are the raw bytes': the caller hashes them)
    }
    return r;
}

int decode(const Options &o, bool to_file, const char *in_path, const char *out_path)
{
    if (to_file && refuse_existing(out_path)) return -1;
    std::vector<uint8_t> in;
    if (!slurp(in_path, in)) { printf("Error: %s file does not exist\n", in_path); return -1; }
    OutFile fout;
    if (to_file && !fout.open(out_path)) { printf("Error: %s file does not exist\n", out_path); return -1; }
    const clock_t t0 = clock();
    Index ix;
    nlzm::index::parse((std::string(in_path) + ".idx").c_str(), ix);
    if (ix.typed() && o.steps_k) { printf("Error: %s.idx is an NLZMIDX 3 index: -steps:K does not decode typed blocks (-elem:E)\n", in_path); return -1; }
    if (o.on_gpu && nlzm_hip_init(0)) return hip_error();
    Found f;
    Decoded r;
    // by the index first; an index that passes its checks and still does not describe these streams (stale, or of another file) is set aside,
    // and the frame headers decide
    for (int attempt = 0; attempt < 2; attempt++) {
        f = find_parts(in, attempt == 0 ? &ix : nullptr, in_path);
        if (ix.typed() && !f.by_index) {            // (only the index says which blocks are byte planes, and of which element size)
            printf("Error: %s.idx (NLZMIDX 3) does not fit this file, and without it the byte planes of its blocks cannot be undone\n", in_path);
            return -1;
        }
        r = Decoded{};
        if (f.parts.empty()) r.rc = -3;
        else if (o.on_gpu && o.steps_k) r = decode_in_steps(f, o.steps_k, fout.f);
        else if (o.on_gpu && f.ix.has_crc() && !to_file && !f.ix.typed()) r = check_on_device(f);
        else if (o.on_gpu) r = decode_on_device(f);
        else r = decode_on_host(f);
        if (r.failed) return -1;
        if (!(f.by_index && (r.index_wrong || r.rc))) break;
        printf("Note: %s.idx does not describe this file's blocks; they are found by their frame headers\n", in_path);
    }
    const size_t k = f.parts.size();
    if (r.rc) { printf("Assert failed: malformed stream (%d)\n", r.rc); fout.done(); return -1; }      // (d leaves the file it opened, empty)
    const bool check_crc = f.by_index && f.ix.has_crc();
    if (check_crc && r.got_crcs.empty()) {
        // one stream, typed blocks, or d -gpu: the bytes are on the host, hashed there block by block
        r.got_crcs.assign(k, 0);
        std::vector<uint64_t> at(k, 0);
        for (size_t i = 1; i < k; i++) at[i] = at[i - 1] + f.ix.raw[i - 1];
        for_each_block(k, [&](size_t i) { r.got_crcs[i] = crc_calc(r.out.data() + at[i], f.ix.raw[i], 0); });
    }
    uint32_t out_crc = 0;
    if (r.out_on_device) for (size_t i = 0; i < k; i++) out_crc = nlzm_hip_crc32_combine(out_crc, r.got_crcs[i], f.ix.raw[i]);
    else { out_crc = crc_calc(r.out.data(), r.out.size(), 0); r.out_size = r.out.size(); }
    printf("Dictionary: %d KB\n", (int)(((1ull << r.hb) + 1023) >> 10));
    printf("Frame: %d KB\n", (int)(((1u << r.fb) + 1023) >> 10));
    if (to_file) { fwrite(r.out.data(), 1, r.out.size(), fout.f); fout.done(); }
    printf("Working... %" PRIu64 " -> %" PRIu64 "\n", (uint64_t)in.size(), r.out_size);
    printf("Done (output CRC32 %X, %.2f sec)\n", out_crc, (clock() - t0) / (double)CLOCKS_PER_SEC);
    bool crc_bad = false;
    if (check_crc) {
        // the index's CRCs against what decoded: every block, then -- where the container is whole -- their combination against the file's
        uint32_t comb = 0;
        for (size_t i = 0; i < k; i++) comb = nlzm_hip_crc32_combine(comb, r.got_crcs[i], f.ix.raw[i]);
        for (size_t i = 0; i < k && !crc_bad; i++)
            if (r.got_crcs[i] != f.ix.crc[i]) { printf("CRC32 MISMATCH in block %zu (index says %08X, decoded %08X)\n", i + 1, f.ix.crc[i], r.got_crcs[i]); crc_bad = true; }
        if (!crc_bad && !f.cut_tail && comb != f.ix.whole) { printf("CRC32 MISMATCH of the whole file (index says %08X, blocks combine to %08X)\n", f.ix.whole, comb); crc_bad = true; }
        if (!crc_bad) printf("CRC32 ok (%zu blocks)\n", k);
        else if (to_file) printf("Note: %s holds what decoded\n", out_path);
    }
    if (f.cut_tail) { printf("Error: the container is cut off inside block %zu (%zu bytes of it present); %zu complete blocks decoded\n", k + 1, f.cut_tail, k); return -2; }
    return crc_bad ? -4 : 0;
}

// ---- x: byte ranges of what a container holds (not in the reference) -----------------------------------------------------------
// The index as `x` needs it: the file itself is not consulted (it may be cut off behind the blocks a range needs), so the checks are structural.
int extract(const char *in_path, const char *out_path, const std::vector<ByteRange> &ranges, bool on_gpu)
{
    if (refuse_existing(out_path)) return -1;
    Index ix;
    nlzm::index::parse((std::string(in_path) + ".idx").c_str(), ix);
    if (ix.typed()) { printf("Error: %s.idx is an NLZMIDX 3 index: x does not read the ranges of typed blocks (-elem:E); d undoes their byte planes\n", in_path); return -1; }
    std::unique_ptr<FILE, int (*)(FILE *)> fin(fopen(in_path, "rb"), fclose);
    if (!fin) { printf("Error: %s file does not exist\n", in_path); return -1; }
    fseeko(fin.get(), 0, SEEK_END);
    const uint64_t file_size = (uint64_t)ftello(fin.get());
    std::vector<uint8_t> whole_file;                // (without an index: the container is read whole and split by its frame headers)
    const bool by_index = nlzm::index::structural(ix, kExtractTakes);
    const clock_t t0 = clock();
    if (on_gpu && nlzm_hip_init(0)) return hip_error();
    std::vector<std::vector<uint8_t>> decoded;      // host path: the needed blocks, whole
    // `count` blocks decoded whole by the host decoder, one thread each: the i-th from its stream into decoded[slot(i)]
    auto decode_blocks = [&](size_t count, auto stream, auto slot) {
        std::vector<int> rcs(count, 0);
        for_each_block(count, [&](size_t i) { uint32_t hb, fb; rcs[i] = decode_stream(stream(i), decoded[slot(i)], &hb, &fb); });
        return rcs;
    };
    if (!by_index) {
        printf("Note: no usable %s.idx; the blocks are found by their frame headers and sized by decoding them\n", in_path);
        ix = Index{};
        whole_file.resize((size_t)file_size);
        fseeko(fin.get(), 0, SEEK_SET);
        if (file_size && fread(whole_file.data(), 1, (size_t)file_size, fin.get()) != (size_t)file_size) { printf("Error: %s could not be read\n", in_path); return -1; }
        if (!nlzm_host::split_streams(Span{ whole_file.data(), whole_file.size() }, SIZE_MAX, ix.len)) { printf("Assert failed: malformed stream (-3)\n"); return -1; }
        ix.off.assign(ix.len.size(), 0);
        for (size_t i = 1; i < ix.len.size(); i++) ix.off[i] = ix.off[i - 1] + ix.len[i - 1];
        ix.raw.assign(ix.off.size(), 0); ix.crc.assign(ix.off.size(), 0);
        if (on_gpu) {
            uint64_t total = 0;
            if (nlzm_hip_decompress_blocks(whole_file.data(), ix.off.back() + ix.len.back(), (uint32_t)ix.off.size(), ix.len.data(), nullptr, nullptr, 0, ix.raw.data(), &total)) return hip_error();
        } else {
            decoded.resize(ix.off.size());
            const std::vector<int> rcs = decode_blocks(ix.off.size(), [&](size_t i) { return Span{ whole_file.data() + ix.off[i], (size_t)ix.len[i] }; }, [](size_t i) { return i; });
            for (size_t i = 0; i < ix.off.size(); i++) {
                if (rcs[i]) { printf("Assert failed: malformed stream (%d)\n", rcs[i]); return -1; }
                ix.raw[i] = decoded[i].size();
            }
        }
    }
    const size_t k = ix.off.size();
    // the library's plan (nlzm_read_plan.h): the ranges checked against what the container holds; need[b], the furthest byte a range wants of block b
    std::vector<uint64_t> off(ranges.size()), len(ranges.size());
    for (size_t r = 0; r < ranges.size(); r++) { off[r] = ranges[r].off; len[r] = ranges[r].len; }
    nlzm::range::Plan plan;
    char why[512];
    if (nlzm::range::make_plan(plan, (uint32_t)k, ix.raw.data(), (uint32_t)ranges.size(), off.data(), len.data(), ~0ull, nlzm::ErrText{ why, sizeof why })) {
        if (plan.bad_range < ranges.size()) printf("Error: range %" PRIu64 ":%" PRIu64 " runs over the %" PRIu64 " bytes the container holds\n", off[plan.bad_range], len[plan.bad_range], plan.total);
        else printf("Error: %s\n", why);
        return -1;
    }
    const std::vector<uint64_t> &start = plan.start, &need = plan.need;
    const uint64_t out_size = plan.dst_len;
    // their streams: only those byte spans of the file, by seek and read
    std::vector<size_t> picked;
    std::vector<uint64_t> sub_off, sub_len, sub_raw, sub_start;
    std::vector<uint32_t> sub_crc;
    std::vector<uint8_t> packed;
    uint64_t packed_len = 0, sub_total = 0;
    for (size_t b = 0; b < k; b++) if (need[b]) {
        picked.push_back(b); sub_off.push_back(packed_len); sub_len.push_back(ix.len[b]); sub_raw.push_back(ix.raw[b]); sub_crc.push_back(ix.crc[b]);
        sub_start.push_back(sub_total);
        packed_len += ix.len[b]; sub_total += ix.raw[b];
    }
    if (by_index || on_gpu) {
        packed.resize((size_t)packed_len);
        for (size_t i = 0; i < picked.size(); i++) {
            const size_t b = picked[i];
            bool ok = ix.off[b] <= file_size && ix.len[b] <= file_size - ix.off[b];
            if (ok && whole_file.empty()) ok = !fseeko(fin.get(), (off_t)ix.off[b], SEEK_SET) && fread(packed.data() + sub_off[i], 1, (size_t)ix.len[b], fin.get()) == (size_t)ix.len[b];
            else if (ok) memcpy(packed.data() + sub_off[i], whole_file.data() + ix.off[b], (size_t)ix.len[b]);
            if (!ok) { printf("Error: the container is cut off inside block %zu, which a range needs\n", b + 1); return -1; }
        }
    }
    fin.reset();
    printf("Blocks: %zu, %zu of them read\n", k, picked.size());
    // a range lies in consecutive blocks, all of them picked but the empty ones: in the picked blocks' contents it starts at
    auto sub_of = [&](const ByteRange &r) {
        if (!r.len) return (uint64_t)0;
        size_t i = 0;
        while (start[picked[i] + 1] <= r.off) i++;
        return sub_start[i] + (r.off - start[picked[i]]);
    };
    std::vector<uint8_t> out((size_t)out_size);
    size_t full = 0;
    long bad_block = -1;
    uint32_t bad_got = 0;
    const bool check_crc = by_index && ix.has_crc();
    for (size_t i = 0; i < picked.size(); i++) full += need[picked[i]] == ix.raw[picked[i]];
    if (on_gpu) {
        for (size_t r = 0; r < ranges.size(); r++) off[r] = sub_of(ranges[r]);
        uint64_t got = 0;
        uint32_t first_bad = (uint32_t)picked.size();
        const int rc = picked.empty() ? 0
                     : nlzm_hip_read_ranges(packed.data(), packed_len, (uint32_t)picked.size(), sub_len.data(), sub_raw.data(), check_crc ? sub_crc.data() : nullptr,
                                            (uint32_t)ranges.size(), off.data(), len.data(), out.data(), out_size, &got, &first_bad);
        if (rc == NLZM_HIP_E_FORMAT || rc == NLZM_HIP_E_CAPACITY) return hip_error("a block does not decode to what its index entry says: ");
        if (rc) return hip_error();
        if (check_crc && first_bad < picked.size()) {
            // (what the block hashes to, for the message: decoded once more on the host, on this path only)
            std::vector<uint8_t> o; uint32_t hb, fb;
            (void)decode_stream(Span{ packed.data() + sub_off[first_bad], (size_t)sub_len[first_bad] }, o, &hb, &fb);
            bad_block = (long)picked[first_bad]; bad_got = crc_calc(o.data(), o.size(), 0);
        }
        nlzm_hip_shutdown();
    } else {
        // the needed blocks decoded whole and sliced
        if (decoded.empty()) {
            decoded.resize(k);
            const std::vector<int> rcs = decode_blocks(picked.size(), [&](size_t i) { return Span{ packed.data() + sub_off[i], (size_t)sub_len[i] }; }, [&](size_t i) { return picked[i]; });
            for (size_t i = 0; i < picked.size(); i++) {
                if (rcs[i]) { printf("Assert failed: malformed stream (%d)\n", rcs[i]); return -1; }
                if (decoded[picked[i]].size() != ix.raw[picked[i]]) {
                    printf("Error: block %zu decodes to %zu bytes, its index entry says %" PRIu64 "\n", picked[i] + 1, decoded[picked[i]].size(), ix.raw[picked[i]]);
                    return -1;
                }
            }
        }
        uint64_t at = 0;
        for (const ByteRange &r : ranges) {
            nlzm::range::for_each_part(start, (uint32_t)k, r.off, r.len, [&](uint32_t b, uint64_t from, uint64_t to) {
                memcpy(out.data() + at + (from - r.off), decoded[b].data() + (from - start[b]), (size_t)(to - from));
            });
            at += r.len;
        }
        for (size_t i = 0; check_crc && i < picked.size() && bad_block < 0; i++) {
            const size_t b = picked[i];
            if (need[b] != ix.raw[b]) continue;
            const uint32_t c = crc_calc(decoded[b].data(), decoded[b].size(), 0);
            if (c != ix.crc[b]) { bad_block = (long)b; bad_got = c; }
        }
    }
    // (x opens its output when it has the bytes, and leaves it: what decoded is what a user can recover)
    FILE *fout = fopen(out_path, "wb");
    if (!fout) { printf("Error: %s file does not exist\n", out_path); return -1; }
    fwrite(out.data(), 1, out.size(), fout);
    fclose(fout);
    printf("Working... %zu ranges -> %" PRIu64 "\n", ranges.size(), out_size);
    printf("Done (output CRC32 %X, %.2f sec)\n", crc_calc(out.data(), out.size(), 0), (clock() - t0) / (double)CLOCKS_PER_SEC);
    if (check_crc) {
        if (bad_block >= 0) {
            printf("CRC32 MISMATCH in block %ld (index says %08X, decoded %08X)\n", bad_block + 1, ix.crc[(size_t)bad_block], bad_got);
            printf("Note: %s holds what decoded\n", out_path);
            return -4;
        }
        printf("CRC32 ok (%zu of %zu blocks read in full)\n", full, picked.size());
    }
    return 0;
}

int hash(const char *in_path, bool on_gpu)
{
    std::vector<uint8_t> in;
    if (!slurp(in_path, in)) { printf("Error: %s file does not exist\n", in_path); return -1; }
    uint32_t crc = 0;
    if (on_gpu) {
        if (nlzm_hip_init(0) || nlzm_hip_crc32(in.data(), in.size(), 0, &crc)) return hip_error();
        nlzm_hip_shutdown();
    } else crc = crc_calc(in.data(), in.size(), 0);
    printf("%X\n", crc);
    return 0;
}

void usage()
{
    printf("Commands:\n"
           "\t[flags] c [input] [output] - Compress input file to output file (best parser)\n"
           "\td [input] [output] - Decompress input file to output file\n"
           "\tt [input] - Decompress input file in memory\n"
           "\th [input] - Calculate CRC32 for input file\n"
           "\t-range:off:len [-range:...] x [input] [output] - (this build) write those byte ranges of what a block container holds; needs [input].idx\n"
           "Flags:\n"
           "\t-window:bits = Maximum window size in bits, default 22 (4 MB), min 15, max 28 (32 KB to 256 MB)\n"
           "\t-blocks:k = (this build) compress k independent blocks, 1 to 65536: as many at once as a launch holds (64), more of them\n"
           "\t            in sets one after another; d/t read the streams back to back\n"
           "\t-cdc:B = (this build) c cuts the blocks by content on the GPU, 2^B bytes on average (B 10 to 30): an edit changes the blocks around it only\n"
           "\t-elem:E = (this build) c compresses every block's byte planes at element size E (2, 4 or 8), alone or with -blocks:k / -cdc:B, and writes NLZMIDX 3; d / t undo them\n"
           "\t-dedup = (this build) with -cdc:B: a block whose bytes an earlier block holds is not compressed again, its stream is a copy (the same container)\n"
           "\t-gpus:g = (this build) the blocks on GPUs 0..g-1 of this node, -blocks:k of them on each (64 at most)\n"
           "\t-verify = (this build) c decodes what it wrote on the GPU, one workgroup per stream, compares it with the input\n"
           "\t          and removes the output if they differ\n"
           "\t-gpu = (this build) d / t decode on the GPU, all blocks of a container at once (without it they run on the host); h hashes there\n"
           "\t-steps:K = (this build) d -gpu / t -gpu decode in steps of K frames per block; d writes every step's bytes as they come\n"
           "\t-crc = (this build) c hashes every block on the GPU and keeps the CRC32s in [output].idx (NLZMIDX 2), for one stream too;\n"
           "\t       d / t compare what they decode with an index that holds CRC32s and exit with status -4 if a block differs\n");
}

// one flag, lower-cased and without its dashes, into the options; false: it is refused, and the message is printed
bool parse_flag(const char *arg, Options &o)
{
    auto clamped = [](const char *digits, int lo, int hi) { const int v = atoi(digits); return (uint32_t)(v < lo ? lo : (v > hi ? hi : v)); };
    unsigned long long v = 0, len = 0;
    const char *p = nullptr;
    if (!strncmp(arg, "window:", 7)) {
        o.hist_bits = clamped(arg + 7, 15, 28);
        printf("Window bits: %d\n", o.hist_bits);
    } else if (!strncmp(arg, "blocks:", 7)) {
        o.nblocks = clamped(arg + 7, 1, (int)nlzm::container::kMaxBlocks);
        printf("Blocks: %d\n", o.nblocks);
    } else if (!strncmp(arg, "gpus:", 5)) {
        o.ngpus = clamped(arg + 5, 1, 64);
        printf("GPUs: %d\n", o.ngpus);
    } else if (!strncmp(arg, "cdc:", 4)) {
        if (!parse_uint(p = arg + 4, 30, v) || *p || v < 10) { printf("Error: -cdc:B takes B from 10 to 30 (blocks of 2^B bytes on average)\n"); return false; }
        o.cdc_bits = (uint32_t)v;
    } else if (!strncmp(arg, "elem:", 5)) {
        if (strcmp(arg + 5, "2") && strcmp(arg + 5, "4") && strcmp(arg + 5, "8")) { printf("Error: -elem:E takes E of 2, 4 or 8 (the bytes of an element)\n"); return false; }
        o.elem = (uint32_t)(arg[5] - '0');
    } else if (!strcmp(arg, "dedup")) {
        o.dedup = true;
    } else if (!strcmp(arg, "verify")) {
        o.verify = true;
    } else if (!strcmp(arg, "crc")) {
        o.with_crc = true;
    } else if (!strcmp(arg, "gpu")) {
        o.on_gpu = true;
    } else if (!strncmp(arg, "steps:", 6) && parse_uint(p = arg + 6, 0xFFFFFFFFull, v) && !*p && v >= 1) {          // 1 .. 2^32 - 1
        o.steps_k = (uint32_t)v;
    } else if (!strncmp(arg, "range:", 6) && parse_uint(p = arg + 6, ~0ull, v) && *p++ == ':' && parse_uint(p, ~0ull, len) && !*p) {
        o.ranges.push_back(ByteRange{ v, len });
    } else {
        printf("Unrecognized flag %s\n", arg);
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    printf("NLZM 1.03 - Written by Nauful (MI355X/gfx950 build)\n");
    // (-blocks:k runs k streams' kernels side by side: the HIP runtime needs more than its default of 4 hardware queues for that, and reads
    //  the variable at the first HIP call -- nlzm_hip_init sets it too, this is for a main that touches HIP before it)
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    crc_init();
    Options o;
    while (argc >= 2 && *argv[1] == '-') {
        char *arg = argv[1];
        argv++; argc--;
        lower(arg);
        while (*arg == '-') ++arg;
        if (!parse_flag(arg, o)) return -1;
    }
    const int cmd = argc >= 2 ? (argv[1][0] | 0x20) : 0;
    if (o.cdc_bits && (o.nblocks > 1 || o.ngpus)) { printf("Error: -cdc:B cuts the blocks by content; it does not go together with -blocks:k or -gpus:g\n"); return -1; }
    if (o.dedup && !o.cdc_bits) { printf("Error: -dedup skips the duplicates among the blocks that -cdc:B cuts; it needs -cdc:B\n"); return -1; }
    if (o.elem && o.ngpus) { printf("Error: -elem:E filters the blocks of one GPU's container; it does not go together with -gpus:g\n"); return -1; }
    if (o.elem) o.with_crc = true;                  // (the index holds the CRC32s of the RAW bytes: what d / t hold the undone planes against)
    if (o.ngpus && o.nblocks > 64) { o.nblocks = 64; printf("Blocks: %d (on each GPU: a launch holds no more)\n", o.nblocks); }
    const bool decodes = (argc == 4 && cmd == 'd') || (argc == 3 && cmd == 't');
    if (o.steps_k && !(o.on_gpu && decodes)) { printf("Error: -steps:K is for d -gpu and t -gpu\n"); return -1; }
    if (argc == 4 && cmd == 'c') {
        if (refuse_existing(argv[3])) return -1;
        const bool one_stream = !o.ngpus && o.nblocks == 1 && !o.verify && !o.cdc_bits && !o.elem;
        return one_stream ? compress_one_stream(o, argv[2], argv[3]) : compress_container(o, argv[2], argv[3]);
    }
    if (decodes) return decode(o, cmd == 'd', argv[2], cmd == 'd' ? argv[3] : nullptr);
    if (argc == 4 && cmd == 'x' && !o.ranges.empty()) return extract(argv[2], argv[3], o.ranges, o.on_gpu);
    if (argc == 3 && cmd == 'h') return hash(argv[2], o.on_gpu);
    usage();
    return 0;
}

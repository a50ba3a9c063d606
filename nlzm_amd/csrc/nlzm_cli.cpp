// nlzm_cli.cpp -- host side of the MI355X build: NLZM's own command line
// (NLZM.cpp:2050-2178) in one file.  `c` runs the compress path on the GPU through
// the C ABI of include/nlzm_hip.h and fails if no gfx950 device is present;
// `d`/`t` decode on the host (the decoder is a serial byte-copy machine and stays
// on the CPU: SURVEY.md 8f-1); `h` prints the CRC32; `x` (not in the reference) writes byte ranges of what
// a block container holds, reading only the blocks they need (host decoder, or nlzm_hip_read_ranges with -gpu).
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
#include <thread>
#include <string>
#include <vector>

#include "../../include/nlzm_hip.h"
#include "nlzm_host_decode.h"
#include "nlzm_read_plan.h"
#include "nlzm_container_plan.h"       // (kMaxBlocks)

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

// ---- host decoder: decode_file (NLZM.cpp:1912-2039), shared with the device decoder's test harness ----------
using nlzm_host::Span;
using nlzm_host::be32;
using nlzm_host::stream_length;
using nlzm_host::decode_stream;

void lower(char *v) { for (; *v; v++) *v = (char)(*v | 0x20); }

// ---- -elem:E: the byte planes of a typed block undone on the host (the rule of nlzm_planes.h restated: y[j m + i] = x[i e + j], the tail as it is) ----
void planes_undo(const uint8_t *y, uint8_t *x, uint64_t n, uint32_t e)
{
    const uint64_t m = n / e;
    for (uint32_t j = 0; j < e; j++) for (uint64_t i = 0; i < m; i++) x[i * e + j] = y[j * m + i];
    for (uint64_t t = e * m; t < n; t++) x[t] = y[t];
}
// does the sidecar index say NLZMIDX 3 (`c -elem:E` wrote it: blocks whose bytes are byte planes)?
bool typed_index(const std::string &path)
{
    FILE *fi = fopen(path.c_str(), "rb");
    if (!fi) return false;
    unsigned ver = 0;
    const bool typed = fscanf(fi, "NLZMIDX %u", &ver) == 1 && ver == 3;
    fclose(fi);
    return typed;
}

// ---- x: byte ranges of what a container holds (not in the reference) -----------------------------------------------------------
struct ByteRange { uint64_t off, len; };

// The sidecar index as `x` needs it: the file itself is not consulted (it may be cut off behind the blocks a range needs), so the checks are
// the structural ones -- no sum that wraps, offsets back to back, lengths summing to the header's n_out and raw lengths to its n_in.
struct Index { std::vector<uint64_t> off, len, raw; std::vector<uint32_t> crc; bool has_crc = false; };
bool read_index(const std::string &path, Index &ix)
{
    FILE *fi = fopen(path.c_str(), "rb");
    if (!fi) return false;
    unsigned ver = 0, k = 0, whole = 0;
    unsigned long long n_in = 0, n_out = 0, expect = 0, raw_sum = 0;
    bool ok = fscanf(fi, "NLZMIDX %u %u %llu %llu", &ver, &k, &n_in, &n_out) == 4 && (ver == 1 || ver == 2) && k >= 1 && k <= 65536;
    if (ok && ver == 2) ok = fscanf(fi, "%x", &whole) == 1;
    for (unsigned i = 0; ok && i < k; i++) {
        unsigned long long off = 0, len = 0, raw = 0;
        unsigned bc = 0;
        ok = fscanf(fi, "%llu %llu %llu", &off, &len, &raw) == 3 && (ver == 1 || fscanf(fi, "%x", &bc) == 1) && off == expect && len >= 8 && len <= n_out - expect &&
             raw <= n_in - raw_sum;
        if (ok) { ix.off.push_back(off); ix.len.push_back(len); ix.raw.push_back(raw); ix.crc.push_back(bc); expect += len; raw_sum += raw; }
    }
    char extra[2];
    if (ok && fscanf(fi, "%1s", extra) == 1) ok = false;       // (fields behind the last block's: not this index)
    fclose(fi);
    ix.has_crc = ver == 2;
    return ok && expect == n_out && raw_sum == n_in;
}

int extract(const char *in_path, const char *out_path, const std::vector<ByteRange> &ranges, bool on_gpu)
{
    if (FILE *probe = fopen(out_path, "rb")) { printf("Error: %s already exists\n", out_path); fclose(probe); return -1; }
    if (typed_index(std::string(in_path) + ".idx")) { printf("Error: %s.idx is an NLZMIDX 3 index: x does not read the ranges of typed blocks (-elem:E); d undoes their byte planes\n", in_path); return -1; }
    FILE *fin = fopen(in_path, "rb");
    if (!fin) { printf("Error: %s file does not exist\n", in_path); return -1; }
    fseeko(fin, 0, SEEK_END);
    const uint64_t file_size = (uint64_t)ftello(fin);
    Index ix;
    std::vector<uint8_t> whole_file;                // (without an index: the container is read whole and split by its frame headers)
    const bool by_index = read_index(std::string(in_path) + ".idx", ix);
    const clock_t t0 = clock();
    if (on_gpu && nlzm_hip_init(0)) { printf("Error: %s\n", nlzm_hip_last_error()); fclose(fin); return -1; }
    std::vector<std::vector<uint8_t>> decoded;      // host path: the needed blocks, whole
    if (!by_index) {
        printf("Note: no usable %s.idx; the blocks are found by their frame headers and sized by decoding them\n", in_path);
        ix = Index{};
        whole_file.resize((size_t)file_size);
        fseeko(fin, 0, SEEK_SET);
        if (file_size && fread(whole_file.data(), 1, (size_t)file_size, fin) != (size_t)file_size) { printf("Error: %s could not be read\n", in_path); fclose(fin); return -1; }
        if (!nlzm_host::split_streams(Span{ whole_file.data(), whole_file.size() }, SIZE_MAX, ix.len)) { printf("Assert failed: malformed stream (-3)\n"); fclose(fin); return -1; }
        ix.off.assign(ix.len.size(), 0);
        for (size_t i = 1; i < ix.len.size(); i++) ix.off[i] = ix.off[i - 1] + ix.len[i - 1];
        ix.raw.assign(ix.off.size(), 0); ix.crc.assign(ix.off.size(), 0);
        if (on_gpu) {
            uint64_t total = 0;
            if (nlzm_hip_decompress_blocks(whole_file.data(), ix.off.back() + ix.len.back(), (uint32_t)ix.off.size(), ix.len.data(), nullptr, nullptr, 0, ix.raw.data(), &total)) {
                printf("Error: %s\n", nlzm_hip_last_error()); fclose(fin); return -1;
            }
        } else {
            decoded.resize(ix.off.size());
            std::vector<int> rcs(ix.off.size(), 0);
            std::vector<std::thread> th;
            for (size_t i = 0; i < ix.off.size(); i++)
                th.emplace_back([&, i] { uint32_t hb, fb; rcs[i] = decode_stream(Span{ whole_file.data() + ix.off[i], (size_t)ix.len[i] }, decoded[i], &hb, &fb); });
            for (auto &t : th) t.join();
            for (size_t i = 0; i < ix.off.size(); i++) {
                if (rcs[i]) { printf("Assert failed: malformed stream (%d)\n", rcs[i]); fclose(fin); return -1; }
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
        fclose(fin); return -1;
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
            if (ok && whole_file.empty()) ok = !fseeko(fin, (off_t)ix.off[b], SEEK_SET) && fread(packed.data() + sub_off[i], 1, (size_t)ix.len[b], fin) == (size_t)ix.len[b];
            else if (ok) memcpy(packed.data() + sub_off[i], whole_file.data() + ix.off[b], (size_t)ix.len[b]);
            if (!ok) { printf("Error: the container is cut off inside block %zu, which a range needs\n", b + 1); fclose(fin); return -1; }
        }
    }
    fclose(fin);
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
    const bool check_crc = by_index && ix.has_crc;
    for (size_t i = 0; i < picked.size(); i++) full += need[picked[i]] == ix.raw[picked[i]];
    if (on_gpu) {
        for (size_t r = 0; r < ranges.size(); r++) off[r] = sub_of(ranges[r]);
        uint64_t got = 0;
        uint32_t first_bad = (uint32_t)picked.size();
        const int rc = picked.empty() ? 0
                     : nlzm_hip_read_ranges(packed.data(), packed_len, (uint32_t)picked.size(), sub_len.data(), sub_raw.data(), check_crc ? sub_crc.data() : nullptr,
                                            (uint32_t)ranges.size(), off.data(), len.data(), out.data(), out_size, &got, &first_bad);
        if (rc == NLZM_HIP_E_FORMAT || rc == NLZM_HIP_E_CAPACITY) { printf("Error: a block does not decode to what its index entry says: %s\n", nlzm_hip_last_error()); return -1; }
        if (rc) { printf("Error: %s\n", nlzm_hip_last_error()); return -1; }
        if (check_crc && first_bad < picked.size()) {
            // (what the block hashes to, for the message: decoded once more on the host, on this path only)
            std::vector<uint8_t> o; uint32_t hb, fb;
            (void)decode_stream(Span{ packed.data() + sub_off[first_bad], (size_t)sub_len[first_bad] }, o, &hb, &fb);
            bad_block = (long)picked[first_bad]; bad_got = crc_calc(o.data(), o.size(), 0);
        }
        nlzm_hip_shutdown();
    } else {
        // the needed blocks decoded whole by the host decoder, one thread per block, and sliced
        if (decoded.empty()) {
            decoded.resize(k);
            std::vector<int> rcs(picked.size(), 0);
            std::vector<std::thread> th;
            for (size_t i = 0; i < picked.size(); i++)
                th.emplace_back([&, i] { uint32_t hb, fb; rcs[i] = decode_stream(Span{ packed.data() + sub_off[i], (size_t)sub_len[i] }, decoded[picked[i]], &hb, &fb); });
            for (auto &t : th) t.join();
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

}  // namespace

int main(int argc, char **argv)
{
    printf("NLZM 1.03 - Written by Nauful (MI355X/gfx950 build)\n");
    // (-blocks:k runs k streams' kernels side by side: the HIP runtime needs more than its default of 4 hardware queues for that, and reads
    //  the variable at the first HIP call -- nlzm_hip_init sets it too, this is for a main that touches HIP before it)
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    crc_init();
    uint32_t hist_bits = 22;                                                      // :2071
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
    while (argc >= 2 && *argv[1] == '-') {
        char *arg = argv[1];
        argv++; argc--;
        lower(arg);
        while (*arg == '-') ++arg;
        if (!strncmp(arg, "window:", 7)) {
            const int v = atoi(arg + 7);
            hist_bits = (uint32_t)(v < 15 ? 15 : (v > 28 ? 28 : v));
            printf("Window bits: %d\n", hist_bits);
        } else if (!strncmp(arg, "blocks:", 7)) {
            const int v = atoi(arg + 7);
            nblocks = (uint32_t)(v < 1 ? 1 : (v > (int)nlzm::container::kMaxBlocks ? (int)nlzm::container::kMaxBlocks : v));
            printf("Blocks: %d\n", nblocks);
        } else if (!strncmp(arg, "gpus:", 5)) {
            const int v = atoi(arg + 5);
            ngpus = (uint32_t)(v < 1 ? 1 : (v > 64 ? 64 : v));
            printf("GPUs: %d\n", ngpus);
        } else if (!strncmp(arg, "cdc:", 4)) {
            // digits and nothing else, 10 .. 30
            unsigned v = 0;
            const char *p = arg + 4;
            bool ok = *p >= '0' && *p <= '9';
            for (; ok && *p >= '0' && *p <= '9'; p++) { v = v * 10 + (unsigned)(*p - '0'); if (v > 30) ok = false; }
            if (!ok || *p || v < 10) { printf("Error: -cdc:B takes B from 10 to 30 (blocks of 2^B bytes on average)\n"); return -1; }
            cdc_bits = v;
        } else if (!strncmp(arg, "elem:", 5)) {
            if (strcmp(arg + 5, "2") && strcmp(arg + 5, "4") && strcmp(arg + 5, "8")) { printf("Error: -elem:E takes E of 2, 4 or 8 (the bytes of an element)\n"); return -1; }
            elem = (uint32_t)(arg[5] - '0');
        } else if (!strcmp(arg, "dedup")) {
            dedup = true;
        } else if (!strcmp(arg, "verify")) {
            verify = true;
        } else if (!strcmp(arg, "crc")) {
            with_crc = true;
        } else if (!strcmp(arg, "gpu")) {
            on_gpu = true;
        } else if (!strncmp(arg, "steps:", 6)) {
            // digits and nothing else, 1 .. 2^32 - 1 (as strict as -range:)
            unsigned long long v = 0;
            const char *p = arg + 6;
            bool ok = *p >= '0' && *p <= '9';
            for (; ok && *p >= '0' && *p <= '9'; p++) { v = v * 10 + (unsigned long long)(*p - '0'); if (v > 0xFFFFFFFFull) ok = false; }
            if (!ok || *p || v < 1) { printf("Unrecognized flag %s\n", arg); return -1; }
            steps_k = (uint32_t)v;
        } else if (!strncmp(arg, "range:", 6)) {
            // digits ':' digits and nothing else; a number that does not fit 64 bits is refused, not saturated
            auto number = [](const char *&p, unsigned long long &v) {
                if (*p < '0' || *p > '9') return false;
                for (v = 0; *p >= '0' && *p <= '9'; p++) {
                    if (v > (~0ull - (unsigned long long)(*p - '0')) / 10) return false;
                    v = v * 10 + (unsigned long long)(*p - '0');
                }
                return true;
            };
            const char *p = arg + 6;
            unsigned long long off = 0, len = 0;
            if (!number(p, off) || *p++ != ':' || !number(p, len) || *p) { printf("Unrecognized flag %s\n", arg); return -1; }
            ranges.push_back(ByteRange{ off, len });
        } else {
            printf("Unrecognized flag %s\n", arg);
            return -1;
        }
    }
    const int cmd = argc >= 2 ? (argv[1][0] | 0x20) : 0;
    if (cdc_bits && (nblocks > 1 || ngpus)) { printf("Error: -cdc:B cuts the blocks by content; it does not go together with -blocks:k or -gpus:g\n"); return -1; }
    if (dedup && !cdc_bits) { printf("Error: -dedup skips the duplicates among the blocks that -cdc:B cuts; it needs -cdc:B\n"); return -1; }
    if (elem && ngpus) { printf("Error: -elem:E filters the blocks of one GPU's container; it does not go together with -gpus:g\n"); return -1; }
    if (elem) with_crc = true;                      // (the index holds the CRC32s of the RAW bytes: what d / t hold the undone planes against)
    if (ngpus && nblocks > 64) { nblocks = 64; printf("Blocks: %d (on each GPU: a launch holds no more)\n", nblocks); }
    if (steps_k && !(on_gpu && ((argc == 4 && cmd == 'd') || (argc == 3 && cmd == 't')))) { printf("Error: -steps:K is for d -gpu and t -gpu\n"); return -1; }
    if (argc == 4 && cmd == 'c') {
        if (FILE *probe = fopen(argv[3], "rb")) { printf("Error: %s already exists\n", argv[3]); fclose(probe); return -1; }
        const bool one_stream = !ngpus && nblocks == 1 && !verify && !cdc_bits && !elem;      // (-verify, -cdc and -elem need the input whole: the one-call path)
        std::vector<uint8_t> in;
        FILE *fin = nullptr;
        uint64_t in_size = 0;
        if (one_stream) {       // read, uploaded and compressed piece by piece (nlzm_hip_feed_*): the file is never whole in host memory
            fin = fopen(argv[2], "rb");
            if (!fin) { printf("Error: %s file does not exist\n", argv[2]); return -1; }
            fseeko(fin, 0, SEEK_END);
            in_size = (uint64_t)ftello(fin);
            fseeko(fin, 0, SEEK_SET);
        } else {
            if (!slurp(argv[2], in)) { printf("Error: %s file does not exist\n", argv[2]); return -1; }
            in_size = in.size();
        }
        FILE *fout = fopen(argv[3], "wb");
        if (!fout) { printf("Error: %s file does not exist\n", argv[3]); if (fin) fclose(fin); return -1; }
        if (!ngpus && nlzm_hip_init(0)) { printf("Error: %s\n", nlzm_hip_last_error()); fclose(fout); remove(argv[3]); return -1; }
        uint32_t nstreams = ngpus ? ngpus * nblocks : nblocks;
        std::vector<uint64_t> boff, braw;           // every block's bytes of the input: cut by content, or the equal partition
        if (cdc_bits) {
            // the cut points from the device, with the default lengths: 2^(B - 2) .. 2^(B + 2) bytes a block (2^31 at most)
            const uint64_t min_len = 1ull << (cdc_bits - 2), max_len = cdc_bits + 2 > 31 ? 1ull << 31 : 1ull << (cdc_bits + 2);
            std::vector<uint64_t> cuts(nlzm::container::kMaxBlocks - 1);
            uint32_t ncuts = 0;
            const int crc = nlzm_hip_cut_points(in.data(), in.size(), cdc_bits, min_len, max_len, cuts.data(), (uint32_t)cuts.size(), &ncuts);
            if (crc == NLZM_HIP_E_CAPACITY) printf("Error: -cdc:%u cuts this input into %" PRIu64 " blocks, a container holds %u at most: raise B\n", cdc_bits, (uint64_t)ncuts + 1, nlzm::container::kMaxBlocks);
            else if (crc) printf("Error: %s\n", nlzm_hip_last_error());
            if (crc) { fclose(fout); remove(argv[3]); return -1; }
            if (elem) {                                 // (whole elements a block: the cuts rounded down, equal ones dropped)
                uint32_t kept = 0;
                for (uint32_t i = 0; i < ncuts; i++) {
                    const uint64_t c = cuts[i] / elem * elem;
                    if (c && (!kept || c > cuts[kept - 1])) cuts[kept++] = c;
                }
                ncuts = kept;
            }
            nstreams = ncuts + 1;
            for (uint32_t i = 0; i < nstreams; i++) {
                const uint64_t lo = i ? cuts[i - 1] : 0, hi = i < ncuts ? cuts[i] : (uint64_t)in.size();
                boff.push_back(lo); braw.push_back(hi - lo);
            }
            printf("Blocks: %u (cut by content)\n", nstreams);
        } else if (!one_stream) {
            uint64_t per = (in.size() + nstreams - 1) / nstreams;
            if (elem) per = (per + elem - 1) / elem * elem;      // (whole elements a block)
            for (uint32_t i = 0; i < nstreams; i++) {
                const uint64_t lo = (uint64_t)i * per < in.size() ? (uint64_t)i * per : in.size(), hi = lo + per < in.size() ? lo + per : in.size();
                boff.push_back(lo); braw.push_back(hi - lo);
            }
        }
        uint32_t hb, fb, cs, feed;
        nlzm_hip_geometry(in_size, hist_bits, &hb, &fb, &cs, &feed);
        {   // the reference's summary (:1755-1759): sizes of its own structures for this window
            const uint32_t c1 = hb < 15 ? 15 : (hb > 17 ? 17 : hb), c2 = hb < 16 ? 16 : (hb > 20 ? 20 : hb), c3 = hb < 16 ? 16 : (hb > 22 ? 22 : hb);
            const uint64_t mf = (4ull << 12) + (8ull << (12 + c1 - 15)) + (4ull << (13 + c2 - 16)) + (8ull << hb) + (4ull << (15 + c3 - 16));
            printf("Model: %d KB\n", 2);
            printf("Parser: %d KB\n", 65);
            printf("Dictionary: %d KB\n", (int)(((1ull << hb) + 1023) >> 10));
            printf("Frame: %d KB\n", (int)(((1u << fb) + 1023) >> 10));
            printf("Dictionary search: %d KB\n", (int)((mf + 1023) >> 10));
        }
        if (nstreams > 1)
            printf("Note: %u independent streams are written back to back; this program's d/t read them, the reference's d "
                   "stops after the first\n", nstreams);
        printf("Working...\r");
        uint64_t out_n = 0;
        const clock_t t0 = clock();
        struct timespec w0, w1;
        clock_gettime(CLOCK_MONOTONIC, &w0);
        if (one_stream) {
            // the reference's loop in big steps: read a piece, hand it over, write the frames that are finished (:1774-1778, :1853, :1870-1885)
            std::vector<uint8_t> piece(16u << 20), obuf(16u << 20);
            uint32_t crc = 0;
            int rc = nlzm_hip_feed_begin(in_size, hist_bits);
            auto drain = [&]() {
                for (uint64_t got = 1; !rc && got;) {
                    rc = nlzm_hip_feed_output(obuf.data(), obuf.size(), &got);
                    if (!rc && got) { fwrite(obuf.data(), 1, (size_t)got, fout); out_n += got; }
                }
            };
            for (uint64_t done = 0; !rc && done < in_size;) {
                const size_t m = (size_t)(in_size - done < piece.size() ? in_size - done : piece.size());
                if (fread(piece.data(), 1, m, fin) != m) { printf("Error: %s could not be read\n", argv[2]); rc = -1; break; }
                if (!with_crc) crc = crc_calc(piece.data(), m, crc);
                rc = nlzm_hip_feed(piece.data(), m);
                done += m;
                drain();
                printf("Working... %" PRIu64 " -> %" PRIu64 "\r", done, out_n);
                fflush(stdout);
            }
            if (!rc) rc = nlzm_hip_feed_finish();
            drain();
            if (!rc && with_crc) rc = nlzm_hip_feed_input_crc32(&crc);      // (the input is whole in HBM and nowhere on the host: hashed where it lies)
            nlzm_hip_feed_end();
            fclose(fin);
            clock_gettime(CLOCK_MONOTONIC, &w1);
            if (rc) { if (rc != -1) printf("Error: %s\n", nlzm_hip_last_error()); fclose(fout); remove(argv[3]); return -1; }
            fclose(fout);
            if (with_crc) {
                const std::string ip = std::string(argv[3]) + ".idx";
                if (FILE *fi = fopen(ip.c_str(), "wb")) {
                    fprintf(fi, "NLZMIDX 2 1 %" PRIu64 " %" PRIu64 " %08X\n0 %" PRIu64 " %" PRIu64 " %08X\n", in_size, out_n, crc, out_n, in_size, crc);
                    fclose(fi);
                    printf("Block index: %s\n", ip.c_str());
                }
            }
            printf("Working... %" PRIu64 " -> %" PRIu64 "\n", in_size, out_n);
            printf("Done (input CRC32 %X, %.2f sec)\n", crc, (double)(w1.tv_sec - w0.tv_sec) + 1e-9 * (double)(w1.tv_nsec - w0.tv_nsec));
            nlzm_hip_shutdown();
            return 0;
        }
        // room for the streams (a guaranteed bound: 9.7 GB at 65,536 blocks).  Not a vector: nothing is filled, and the pages behind the streams' end are never touched
        const size_t out_room = ngpus ? (size_t)nlzm_hip_compress_bound(in.size()) + (size_t)nstreams * (16 + 131072)
                              : cdc_bits || elem ? (size_t)nlzm_hip_compress_ranges_bound(nstreams, braw.data()) : (size_t)nlzm_hip_compress_blocks_bound(in.size(), nblocks);
        struct Room { uint8_t *p; size_t n; uint8_t *data() const { return p; } size_t size() const { return n; } ~Room() { free(p); } } out{ (uint8_t *)malloc(out_room ? out_room : 1), out_room };
        if (!out.data()) { printf("Error: no memory for %zu bytes of output\n", out_room); fclose(fout); remove(argv[3]); return -1; }
        std::vector<uint64_t> blen(nstreams);
        std::vector<int> devs;
        for (uint32_t d = 0; d < ngpus; d++) devs.push_back((int)d);
        if (dedup && nlzm_hip_set_option("dedup_ranges", 1)) { printf("Error: %s\n", nlzm_hip_last_error()); fclose(fout); remove(argv[3]); return -1; }
        const std::vector<uint8_t> elems(nstreams, (uint8_t)elem);
        const int rc = elem ? nlzm_hip_compress_ranges_typed(in.data(), in.size(), nstreams, boff.data(), braw.data(), elems.data(), hist_bits, out.data(), out.size(), blen.data(), &out_n)
                     : cdc_bits ? nlzm_hip_compress_ranges(in.data(), in.size(), nstreams, boff.data(), braw.data(), hist_bits, out.data(), out.size(), blen.data(), &out_n)
                     : ngpus ? nlzm_hip_compress_blocks_multi(devs.data(), ngpus, nblocks, in.data(), in.size(), hist_bits, out.data(), out.size(), blen.data(), &out_n)
                     : nblocks > 1 ? nlzm_hip_compress_blocks(in.data(), in.size(), nblocks, hist_bits, out.data(), out.size(), blen.data(), &out_n)
                                   : nlzm_hip_compress(in.data(), in.size(), hist_bits, out.data(), out.size(), &out_n);
        clock_gettime(CLOCK_MONOTONIC, &w1);
        (void)t0;
        if (rc) { printf("Error: %s\n", nlzm_hip_last_error()); fclose(fout); remove(argv[3]); return -1; }
        if (nstreams == 1) blen[0] = out_n;
        if (dedup) {        // (the finder's counters of the call: the blocks that were another's copy, and their bytes)
            uint64_t distinct = nstreams, dup_bytes = 0;
            (void)nlzm_hip_get_counter("dedup_distinct", &distinct);
            (void)nlzm_hip_get_counter("dedup_dup_bytes", &dup_bytes);
            printf("Duplicates: %" PRIu64 " of %u blocks (%" PRIu64 " bytes) not compressed again\n", (uint64_t)nstreams - distinct, nstreams, dup_bytes);
        }
        if (verify) {
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
            if (vrc) { printf("Error: verify: %s\n", nlzm_hip_last_error()); fclose(fout); remove(argv[3]); return -1; }
            if (!NLZM_HIP_VERIFY_EQUAL(first, decoded, (uint64_t)in.size())) {
                if (first < in.size() && first < decoded) printf("Verify FAILED: the stream decodes to something else from offset %" PRIu64 "; %s removed\n", first, argv[3]);
                else printf("Verify FAILED: the stream decodes to %" PRIu64 " bytes, the input has %" PRIu64 " (equal up to offset %" PRIu64 "); %s removed\n", decoded, (uint64_t)in.size(), first, argv[3]);
                fclose(fout); remove(argv[3]);
                return -3;
            }
            uint64_t dev_us = 0;
            (void)nlzm_hip_get_counter("decode_us", &dev_us);
            printf("Verified (%.2f sec, %.2f of them decoding on the device)\n", (double)(v1.tv_sec - v0.tv_sec) + 1e-9 * (double)(v1.tv_nsec - v0.tv_nsec), 1e-6 * (double)dev_us);
        }
        // -crc: every block's CRC32 from the device, on a re-upload of the input as -verify makes one; the whole file's is their combination
        std::vector<uint32_t> bcrc(nstreams, 0);
        uint32_t whole = 0;
        if (with_crc) {
            int crc_rc = ngpus ? nlzm_hip_init(0) : 0;
            if (!crc_rc) crc_rc = nlzm_hip_crc32_ranges(in.data(), in.size(), nstreams, boff.data(), braw.data(), bcrc.data());
            if (crc_rc) { printf("Error: crc: %s\n", nlzm_hip_last_error()); fclose(fout); remove(argv[3]); return -1; }
            for (uint32_t i = 0; i < nstreams; i++) whole = nlzm_hip_crc32_combine(whole, bcrc[i], braw[i]);
        }
        fwrite(out.data(), 1, (size_t)out_n, fout);
        fclose(fout);
        if (nstreams > 1 || with_crc || cdc_bits || elem) {
            // the block index, a sidecar: where every block's stream starts, how long it is and how many input bytes it holds.  The
            // streams stay self-delimiting -- the index only saves d/t the hop over every frame header of every block before the parallel decode can
            // start, and keeps the later blocks' boundaries when the container is damaged inside an earlier one.
            const std::string ip = std::string(argv[3]) + ".idx";
            if (FILE *fi = fopen(ip.c_str(), "wb")) {
                if (elem) fprintf(fi, "NLZMIDX 3 %u %" PRIu64 " %" PRIu64 " %08X\n", nstreams, (uint64_t)in.size(), out_n, whole);
                else if (with_crc) fprintf(fi, "NLZMIDX 2 %u %" PRIu64 " %" PRIu64 " %08X\n", nstreams, (uint64_t)in.size(), out_n, whole);
                else fprintf(fi, "NLZMIDX 1 %u %" PRIu64 " %" PRIu64 "\n", nstreams, (uint64_t)in.size(), out_n);
                uint64_t off = 0;
                for (uint32_t i = 0; i < nstreams; i++) {       // (each block's raw length its true one: the equal partition's, or the content's)
                    if (elem) fprintf(fi, "%" PRIu64 " %" PRIu64 " %" PRIu64 " %08X %u\n", off, blen[i], braw[i], bcrc[i], elem);
                    else if (with_crc) fprintf(fi, "%" PRIu64 " %" PRIu64 " %" PRIu64 " %08X\n", off, blen[i], braw[i], bcrc[i]);
                    else fprintf(fi, "%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", off, blen[i], braw[i]);
                    off += blen[i];
                }
                fclose(fi);
                printf("Block index: %s\n", ip.c_str());
            }
        }
        printf("Working... %" PRIu64 " -> %" PRIu64 "\n", (uint64_t)in.size(), out_n);
        printf("Done (input CRC32 %X, %.2f sec)\n", with_crc ? whole : crc_calc(in.data(), in.size(), 0),
               (double)(w1.tv_sec - w0.tv_sec) + 1e-9 * (double)(w1.tv_nsec - w0.tv_nsec));
        nlzm_hip_shutdown();
    } else if ((argc == 4 && cmd == 'd') || (argc == 3 && cmd == 't')) {
        if (cmd == 'd') {
            if (FILE *probe = fopen(argv[3], "rb")) { printf("Error: %s already exists\n", argv[3]); fclose(probe); return -1; }
        }
        std::vector<uint8_t> in, out;
        if (!slurp(argv[2], in)) { printf("Error: %s file does not exist\n", argv[2]); return -1; }
        FILE *fout = nullptr;
        if (cmd == 'd') {
            fout = fopen(argv[3], "wb");
            if (!fout) { printf("Error: %s file does not exist\n", argv[3]); return -1; }
        }
        uint32_t hb = 0, fb = 0;
        const clock_t t0 = clock();
        // one stream (the reference's format), or several back to back (block mode): found by hopping over the frames,
        // decoded on a host thread each, written in order
        std::vector<Span> parts;
        std::vector<uint64_t> raws;                 // (by index) the input bytes every block holds
        std::vector<uint8_t> idx_elems;             // (by a version-3 index) every block's element size: its bytes are byte planes
        std::vector<uint32_t> idx_crcs;             // (by a version-2 or -3 index) every block's CRC32, and the whole file's
        uint32_t idx_whole = 0;
        bool idx_has_crc = false;
        size_t cut_tail = 0;
        bool by_index = false;
        auto find_parts = [&](bool use_index) {
            parts.clear(); raws.clear(); idx_crcs.clear(); idx_elems.clear(); cut_tail = 0; by_index = false; idx_has_crc = false;
            // the sidecar index of a block container, if it is there and fits the file: the blocks' boundaries without hopping over their frames
            const std::string ip = std::string(argv[2]) + ".idx";
            FILE *fi = use_index ? fopen(ip.c_str(), "rb") : nullptr;
            if (fi) {
                unsigned ver = 0, k = 0;
                unsigned long long n_in = 0, n_out = 0;
                std::vector<Span> idx;
                std::vector<uint64_t> idx_raw;
                std::vector<uint32_t> idx_crc;
                std::vector<uint8_t> idx_elem;
                unsigned whole = 0;
                bool ok = fscanf(fi, "NLZMIDX %u %u %llu %llu", &ver, &k, &n_in, &n_out) == 4 && (ver >= 1 && ver <= 3) && k >= 1 && k <= 4096 && n_out >= in.size();
                if (ok && ver >= 2) ok = fscanf(fi, "%x", &whole) == 1;         // (version 2: version 1 and a CRC32 behind the header's and every block's fields)
                unsigned long long expect = 0, raw_sum = 0;
                bool cut = false;
                for (unsigned i = 0; ok && i < k && !cut; i++) {
                    unsigned long long off = 0, len = 0, raw = 0;
                    unsigned bc = 0, be = 1;
                    ok = fscanf(fi, "%llu %llu %llu", &off, &len, &raw) == 3 && (ver == 1 || fscanf(fi, "%x", &bc) == 1) && (ver < 3 || (fscanf(fi, "%u", &be) == 1 && (be == 1 || be == 2 || be == 4 || be == 8))) &&
                         off == expect && len >= 8 && off <= in.size() && raw <= n_in - raw_sum;
                    if (ok && len > in.size() - off) { cut = true; break; }      // (the file ends inside this block: the ones in front of it are whole; no off + len, which can wrap)
                    // (a block's stream starts with its header and ends with its terminator, :1915-1921, :646-648)
                    if (ok) ok = in[off] == 0 && in[off + 1] >= 10 && in[off + 1] <= 28 && be32(&in[off + len - 4]) == 0;
                    if (ok) { idx.push_back(Span{ in.data() + off, (size_t)len }); idx_raw.push_back(raw); idx_crc.push_back(bc); idx_elem.push_back((uint8_t)be); expect = off + len; raw_sum += raw; }
                }
                fclose(fi);
                if (ok && !idx.empty() && (cut || (expect == in.size() && n_out == in.size() && raw_sum == n_in))) {
                    parts = idx; raws = idx_raw; by_index = true;
                    if (ver >= 2) { idx_crcs = idx_crc; idx_whole = whole; idx_has_crc = true; }
                    if (ver == 3) idx_elems = idx_elem;
                    if (cut) cut_tail = in.size() - (size_t)expect;
                } else printf("Note: %s does not fit this file; the blocks are found by their frame headers\n", ip.c_str());
            }
            for (size_t pos = 0; !by_index && pos < in.size();) {
                const Span rest{ in.data() + pos, in.size() - pos };
                const size_t len = stream_length(rest);
                if (!len) {
                    // what follows is not a stream: the reference stops at the first terminator (:646-648) and so do we;
                    // a container that is cut off inside its first stream is malformed
                    if (parts.empty()) break;
                    // a further stream header (:1915-1921: hist_bits, frame_bits, both big-endian 16-bit) with a frame that is cut off:
                    // the complete streams are decoded and written, and the exit status says that the container was cut
                    const bool header = rest.n >= 4 && rest.p[0] == 0 && rest.p[1] >= 10 && rest.p[1] <= 28 && rest.p[2] == 0 && rest.p[3] >= 12 && rest.p[3] <= 20;
                    if (header) cut_tail = rest.n;
                    else printf("Note: %zu bytes after the last stream ignored\n", rest.n);
                    break;
                }
                parts.push_back(Span{ rest.p, len });
                pos += len;
            }
        };
        const bool typed_idx = typed_index(std::string(argv[2]) + ".idx");
        if (typed_idx && steps_k) { printf("Error: %s.idx is an NLZMIDX 3 index: -steps:K does not decode typed blocks (-elem:E)\n", argv[2]); if (fout) { fclose(fout); remove(argv[3]); } return -1; }
        if (on_gpu && nlzm_hip_init(0)) { printf("Error: %s\n", nlzm_hip_last_error()); if (fout) { fclose(fout); remove(argv[3]); } return -1; }
        int rc = 0;
        std::vector<uint32_t> got_crcs;             // what the blocks decoded to hash to (where a version-2 index gives CRCs to hold against)
        uint64_t out_size = 0;
        bool out_on_device = false;                 // t -gpu with a version-2 index: decoded and hashed on the device, nothing came back
        for (int attempt = 0; attempt < 2; attempt++) {
            find_parts(attempt == 0);
            if (typed_idx && !by_index) {           // (only the index says which blocks are byte planes, and of which element size)
                printf("Error: %s.idx (NLZMIDX 3) does not fit this file, and without it the byte planes of its blocks cannot be undone\n", argv[2]);
                if (fout) { fclose(fout); remove(argv[3]); }
                return -1;
            }
            const bool typed = !idx_elems.empty();
            out.clear(); got_crcs.clear(); out_on_device = false; out_size = 0;
            rc = parts.empty() ? -3 : 0;
            bool index_wrong = false;               // a block did not decode to the bytes its index entry says it holds
            if (!rc && on_gpu && steps_k) {
                // the same decode in steps of K frames per block (nlzm_hip_decode_*): after every step each block's new bytes are fetched, hashed and --
                // d -- written at the block's offset, so the host holds one step's output at a time
                const uint32_t k = (uint32_t)parts.size();
                std::vector<uint64_t> blen(k), raw(k), at(k, 0), done(k, 0), had(k, 0);
                for (uint32_t i = 0; i < k; i++) blen[i] = parts[i].n;
                const uint64_t src_len = (uint64_t)(parts.back().p + parts.back().n - parts[0].p);
                uint64_t total = 0, launches = 0;
                int drc = 0;
                if (by_index) raw = raws;
                else drc = nlzm_hip_decompress_blocks(parts[0].p, src_len, k, blen.data(), nullptr, nullptr, 0, raw.data(), &total);      // (no lengths anywhere in the format: a size pass)
                for (uint32_t i = 1; i < k; i++) at[i] = at[i - 1] + raw[i - 1];
                if (!drc) drc = nlzm_hip_decode_begin(parts[0].p, src_len, k, blen.data(), raw.data(), 0);
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
                if (by_index && (drc == NLZM_HIP_E_CAPACITY || drc == NLZM_HIP_E_FORMAT || drc == NLZM_HIP_E_NOMEM)) { index_wrong = true; drc = 0; }
                if (drc == NLZM_HIP_E_FORMAT) rc = -7;
                else if (drc) { printf("Error: %s\n", nlzm_hip_last_error()); if (fout) { fclose(fout); remove(argv[3]); } return -1; }
                hb = parts[0].p[1]; fb = parts[0].p[3];
                // (a decode that did not come to its end leaves nothing of what its steps wrote: the one-call path writes nothing then either)
                if ((index_wrong || rc) && fout) { fflush(fout); if (ftruncate(fileno(fout), 0)) {} fseeko(fout, 0, SEEK_SET); }
                if (!index_wrong && !rc) {
                    if (k > 1) printf("Blocks: %d\n", (int)k);
                    printf("Steps: %u frames, %" PRIu64 " launches\n", steps_k, launches);
                    if (fout) { fflush(fout); if (ftruncate(fileno(fout), (off_t)total)) {} fseeko(fout, 0, SEEK_END); }
                    raws = raw; got_crcs = crcs; out_size = total; out_on_device = true;        // (nothing of the output is left on the host: its CRC32 is the blocks' combined)
                }
            } else if (!rc && on_gpu && idx_has_crc && cmd == 't' && !typed) {
                // nlzm_hip_check: decoded into a buffer on the device, every block bounded by its index entry, and hashed there
                const uint32_t k = (uint32_t)parts.size();
                std::vector<uint64_t> blen(k), raw(k);
                for (uint32_t i = 0; i < k; i++) blen[i] = parts[i].n;
                const uint64_t src_len = (uint64_t)(parts.back().p + parts.back().n - parts[0].p);
                uint32_t first_bad = k;
                got_crcs.assign(k, 0);
                int drc = nlzm_hip_check(parts[0].p, src_len, k, blen.data(), raws.data(), idx_crcs.data(), &first_bad, got_crcs.data());
                if (!drc && first_bad < k) {
                    // a wrong length or a wrong CRC?  The blocks' own lengths say (a size pass; only a container that fails pays for it)
                    uint64_t total = 0;
                    drc = nlzm_hip_decompress_blocks(parts[0].p, src_len, k, blen.data(), nullptr, nullptr, 0, raw.data(), &total);
                    for (uint32_t i = 0; !drc && i < k; i++) if (raw[i] != raws[i]) index_wrong = true;
                }
                if (drc == NLZM_HIP_E_NOMEM) { index_wrong = true; drc = 0; }
                if (drc == NLZM_HIP_E_FORMAT) rc = -7;
                else if (drc) { printf("Error: %s\n", nlzm_hip_last_error()); return -1; }
                hb = parts[0].p[1]; fb = parts[0].p[3];
                for (uint32_t i = 0; i < k; i++) out_size += raws[i];
                out_on_device = true;
                if (!index_wrong && !rc && k > 1) printf("Blocks: %d\n", (int)k);
                if (index_wrong || rc) { out_size = 0; got_crcs.clear(); }
            } else if (!rc && on_gpu) {
                // all blocks at once on the device, one workgroup each; boundaries from above, raw lengths from the index where it gave them
                std::vector<uint64_t> blen(parts.size()), raw(parts.size());
                for (size_t i = 0; i < parts.size(); i++) blen[i] = parts[i].n;
                const uint64_t src_len = (uint64_t)(parts.back().p + parts.back().n - parts[0].p);
                uint64_t total = 0;
                int drc = 0;
                if (by_index) {
                    // the index says what every block holds: one decode pass, every block bounded by its entry -- a block that decodes to more
                    // (NLZM_HIP_E_CAPACITY) or to less (NLZM_HIP_E_FORMAT) than that shows the index to be wrong, and the frame headers decide
                    // (the sizes are the index's word and nothing else yet: an index that asks for more memory than the host or the device has is a
                    //  wrong index, not a reason to die)
                    for (size_t i = 0; i < parts.size(); i++) total += raws[i];
                    bool room = true;
                    try { out.resize((size_t)total); } catch (const std::exception &) { room = false; }
                    if (room && typed) drc = nlzm_hip_decompress_blocks_typed(parts[0].p, src_len, (uint32_t)parts.size(), blen.data(), raws.data(), idx_elems.data(), out.data(), total, raw.data(), &total);
                    else if (room) drc = nlzm_hip_decompress_blocks(parts[0].p, src_len, (uint32_t)parts.size(), blen.data(), raws.data(), out.data(), total, raw.data(), &total);
                    if (!room || drc == NLZM_HIP_E_CAPACITY || drc == NLZM_HIP_E_FORMAT || drc == NLZM_HIP_E_NOMEM) { index_wrong = true; drc = 0; std::vector<uint8_t>().swap(out); }
                } else {
                    // no lengths anywhere in the format: a size pass, then the decode
                    drc = nlzm_hip_decompress_blocks(parts[0].p, src_len, (uint32_t)parts.size(), blen.data(), nullptr, nullptr, 0, raw.data(), &total);
                    if (!drc) {
                        out.resize((size_t)total);
                        drc = nlzm_hip_decompress_blocks(parts[0].p, src_len, (uint32_t)parts.size(), blen.data(), raw.data(), out.data(), total, nullptr, &total);
                    }
                }
                if (drc == NLZM_HIP_E_FORMAT) rc = -7;
                else if (drc) { printf("Error: %s\n", nlzm_hip_last_error()); if (fout) { fclose(fout); remove(argv[3]); } return -1; }
                hb = parts[0].p[1]; fb = parts[0].p[3];
                if (parts.size() > 1) printf("Blocks: %d\n", (int)parts.size());
            } else if (parts.size() == 1) {
                rc = decode_stream(parts[0], out, &hb, &fb);
                if (!rc && by_index && out.size() != raws[0]) index_wrong = true;
            } else if (!rc) {
                std::vector<std::vector<uint8_t>> outs(parts.size());
                std::vector<int> rcs(parts.size(), 0);
                std::vector<uint32_t> hbs(parts.size(), 0), fbs(parts.size(), 0);
                std::vector<std::thread> th;
                if (idx_has_crc) got_crcs.assign(parts.size(), 0);
                for (size_t i = 0; i < parts.size(); i++)
                    th.emplace_back([&, i] {
                        rcs[i] = decode_stream(parts[i], outs[i], &hbs[i], &fbs[i]);
                        if (!rcs[i] && idx_has_crc) got_crcs[i] = crc_calc(outs[i].data(), outs[i].size(), 0);
                    });
                for (auto &t : th) t.join();
                for (size_t i = 0; i < parts.size() && !rc; i++) {
                    rc = rcs[i];
                    if (!rc && by_index && outs[i].size() != raws[i]) index_wrong = true;
                    out.insert(out.end(), outs[i].begin(), outs[i].end());
                }
                hb = hbs[0]; fb = fbs[0];
                if (!index_wrong) printf("Blocks: %d\n", (int)parts.size());
            }
            if (typed && !on_gpu && !rc && !index_wrong) {
                // host-only: the planes undone block by block, by the rule restated above; the CRC32s are the raw bytes', hashed below
                std::vector<uint8_t> raw_bytes(out.size());
                std::vector<std::thread> th;
                uint64_t at = 0;
                for (size_t i = 0; i < parts.size(); i++) { th.emplace_back([&, i, at] { planes_undo(out.data() + at, raw_bytes.data() + at, raws[i], idx_elems[i]); }); at += raws[i]; }
                for (auto &t : th) t.join();
                out.swap(raw_bytes);
                got_crcs.clear();
            }
            if (!(by_index && (index_wrong || rc))) break;
            // the index passed its checks and still does not describe these streams (stale, or of another file): the frame headers decide
            printf("Note: %s.idx does not describe this file's blocks; they are found by their frame headers\n", argv[2]);
        }
        if (rc) { printf("Assert failed: malformed stream (%d)\n", rc); if (fout) fclose(fout); return -1; }
        const bool check_crc = by_index && idx_has_crc;
        if (check_crc && got_crcs.empty()) {
            // one stream, or d -gpu: the bytes are on the host, hashed there block by block
            got_crcs.assign(parts.size(), 0);
            std::vector<std::thread> th;
            uint64_t at = 0;
            for (size_t i = 0; i < parts.size(); i++) { th.emplace_back([&, i, at] { got_crcs[i] = crc_calc(out.data() + at, raws[i], 0); }); at += raws[i]; }
            for (auto &t : th) t.join();
        }
        uint32_t out_crc = 0;
        if (out_on_device) for (size_t i = 0; i < parts.size(); i++) out_crc = nlzm_hip_crc32_combine(out_crc, got_crcs[i], raws[i]);
        else { out_crc = crc_calc(out.data(), out.size(), 0); out_size = out.size(); }
        printf("Dictionary: %d KB\n", (int)(((1ull << hb) + 1023) >> 10));
        printf("Frame: %d KB\n", (int)(((1u << fb) + 1023) >> 10));
        if (fout) { fwrite(out.data(), 1, out.size(), fout); fclose(fout); }
        printf("Working... %" PRIu64 " -> %" PRIu64 "\n", (uint64_t)in.size(), out_size);
        printf("Done (output CRC32 %X, %.2f sec)\n", out_crc, (clock() - t0) / (double)CLOCKS_PER_SEC);
        bool crc_bad = false;
        if (check_crc) {
            // the index's CRCs against what decoded: every block, then -- where the container is whole -- their combination against the file's
            uint32_t comb = 0;
            for (size_t i = 0; i < parts.size(); i++) comb = nlzm_hip_crc32_combine(comb, got_crcs[i], raws[i]);
            for (size_t i = 0; i < parts.size() && !crc_bad; i++)
                if (got_crcs[i] != idx_crcs[i]) { printf("CRC32 MISMATCH in block %zu (index says %08X, decoded %08X)\n", i + 1, idx_crcs[i], got_crcs[i]); crc_bad = true; }
            if (!crc_bad && !cut_tail && comb != idx_whole) { printf("CRC32 MISMATCH of the whole file (index says %08X, blocks combine to %08X)\n", idx_whole, comb); crc_bad = true; }
            if (!crc_bad) printf("CRC32 ok (%zu blocks)\n", parts.size());
            else if (fout) printf("Note: %s holds what decoded\n", argv[3]);
        }
        if (cut_tail) { printf("Error: the container is cut off inside block %zu (%zu bytes of it present); %zu complete blocks decoded\n", parts.size() + 1, cut_tail, parts.size()); return -2; }
        if (crc_bad) return -4;
    } else if (argc == 4 && cmd == 'x' && !ranges.empty()) {
        return extract(argv[2], argv[3], ranges, on_gpu);
    } else if (argc == 3 && cmd == 'h') {
        std::vector<uint8_t> in;
        if (!slurp(argv[2], in)) { printf("Error: %s file does not exist\n", argv[2]); return -1; }
        uint32_t crc = 0;
        if (on_gpu) {
            if (nlzm_hip_init(0) || nlzm_hip_crc32(in.data(), in.size(), 0, &crc)) { printf("Error: %s\n", nlzm_hip_last_error()); return -1; }
            nlzm_hip_shutdown();
        } else crc = crc_calc(in.data(), in.size(), 0);
        printf("%X\n", crc);
    } else {
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
    return 0;
}

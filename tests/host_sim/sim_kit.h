// sim_kit.h -- what the CPU harnesses of this directory share: buffers that a read or write outside them cannot leave unnoticed, and
// whole-file input and output.  TEST HARNESS ONLY.
//
// A role promises that its reads stay inside [src, src + len) and its writes inside [dst, dst + cap).  The harnesses hold it to that with
// the pages themselves: a buffer lies in a mapping between PROT_NONE pages, so an access that leaves the mapping is a SIGSEGV of the
// harness -- host code, which is where faults belong -- and what the pages enclose beside the buffer is a canary that intact() checks.
// A program that makes such a buffer names itself for the one message this file prints: const char simkit::kProgram[] = "crc_sim";
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

namespace simkit {

extern const char kProgram[];

constexpr size_t kCanary = 4096;
constexpr uint8_t kPoison = 0xA5;

inline size_t page() { return (size_t)sysconf(_SC_PAGESIZE); }
inline size_t pages_for(size_t bytes) { return (bytes + page() - 1) / page() * page(); }

// One mapping: a PROT_NONE page, `room` bytes (a multiple of the page size), a PROT_NONE page, `room` bytes, ... a PROT_NONE page; region i is
// [lo(i), hi(i)).  Several regions in one mapping are for roles whose sources are offsets from one base.
struct Regions {
    uint8_t *base = nullptr;
    size_t room = 0, stride = 0, len = 0;
    Regions() = default;
    Regions(const Regions &) = delete;
    Regions &operator=(const Regions &) = delete;
    ~Regions() { drop(); }
    void drop() { if (base) munmap(base, len); base = nullptr; }
    void make(size_t count, size_t bytes)
    {
        drop();
        const size_t pg = page();
        room = pages_for(bytes); stride = room + pg; len = count * stride + pg;
        base = (uint8_t *)mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        bool ok = base != MAP_FAILED;
        for (size_t i = 0; ok && i <= count; i++) ok = !mprotect(base + i * stride, pg, PROT_NONE);
        if (!ok) { fprintf(stderr, "%s: no guarded buffer\n", kProgram); exit(2); }
    }
    uint8_t *lo(size_t i) const { return base + i * stride + page(); }
    uint8_t *hi(size_t i) const { return lo(i) + room; }
};

// One region between two PROT_NONE pages: [lo, hi).
//   make(bytes): `bytes` rounded up to pages, as the mapping comes (zeroes); the caller places its data at lo + align or at hi - n.
//   make(bytes, misalign, fill, place): a buffer of `bytes` bytes of `fill` inside a region with room for a canary on either side, all of
//       it poison but the buffer -- kMid: the buffer `misalign` bytes behind a canary (a page's start plus 4096: misalign is its address
//       modulo 64 and 16), canaries on both sides; kFront: its first byte right behind the page in front; kBack: its last byte flush against
//       the page behind (the canary is then on the side where no page can sit).
enum Place { kMid, kFront, kBack };
struct Guarded {
    Regions map;
    uint8_t *lo = nullptr, *hi = nullptr, *q = nullptr;      // [lo, hi): readable and writable; q: the buffer
    size_t n = 0;
    void make(size_t bytes)
    {
        map.make(1, bytes);
        lo = q = map.lo(0); hi = map.hi(0); n = map.room;
    }
    void make(size_t bytes, size_t misalign, uint8_t fill, Place place = kMid)
    {
        make(bytes + 2 * kCanary + 64);
        n = bytes;
        memset(lo, kPoison, map.room);
        q = place == kFront ? lo : place == kBack ? hi - bytes : lo + kCanary + misalign;
        memset(q, fill, bytes);
    }
    uint8_t *p() { return q; }
    bool intact() const
    {
        for (const uint8_t *c = lo; c < q; c++) if (*c != kPoison) return false;
        for (const uint8_t *c = q + n; c < hi; c++) if (*c != kPoison) return false;
        return true;
    }
};

// a buffer of n bytes on the heap, `misalign` bytes behind a 64-byte boundary, between two canaries
struct Canaried {
    std::vector<uint8_t> mem;
    size_t off = 0, n = 0;
    void make(size_t bytes, size_t misalign, uint8_t fill)
    {
        n = bytes;
        mem.assign(2 * kCanary + bytes + 64, kPoison);
        off = kCanary + ((64 - ((uintptr_t)mem.data() + kCanary) % 64) % 64) + misalign;
        memset(mem.data() + off, fill, bytes);
    }
    uint8_t *p() { return mem.data() + off; }
    bool intact() const
    {
        for (size_t i = 0; i < off; i++) if (mem[i] != kPoison) return false;
        for (size_t i = off + n; i < mem.size(); i++) if (mem[i] != kPoison) return false;
        return true;
    }
};

inline std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> b;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    b.resize((size_t)sz);
    if (sz && fread(b.data(), 1, (size_t)sz, f) != (size_t)sz) { fprintf(stderr, "short read\n"); exit(2); }
    fclose(f);
    return b;
}
inline void spill(const char *path, const void *p, size_t bytes)
{
    FILE *f = fopen(path, "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    fclose(f);
}

}  // namespace simkit

// A stand-alone host program for the sanitizers: the layout arithmetic of phmm_staging.hpp -- StageLayout's slots, the copy-in
// and the hand-over, out_or_scratch -- with plain heap blocks of exactly `total` bytes standing in for the pinned mirror and the
// device buffers, so an offset or a size that is off by anything is a heap overflow the sanitizer reports.  With no device it
// also checks how DeviceScratch::reserve fails and when it allocates nothing.  Build and run (no GPU needed):
// make -C lorikeet_amd/csrc staging_host_check
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "phmm_staging.hpp"

namespace phmm_host {
void set_create_error(const std::string &) {}
}  // namespace phmm_host

using namespace phmm_host;

namespace {

int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        ++failures;
        fprintf(stderr, "FAILED: %s\n", what);
    }
}

template <class T>
std::vector<T> iota(size_t n, T first) {
    std::vector<T> v(n);
    std::iota(v.begin(), v.end(), first);
    return v;
}

// a StagingBuffer over two heap blocks of exactly L.total bytes: `host` the mirror, `dev` what a kernel would see
struct Blocks {
    std::vector<char> host, dev;
    StagingBuffer W;
    explicit Blocks(const StageLayout &L) : host(L.total, 0x55), dev(L.total, 0x66) {
        W.host = host.data();
        W.dev = dev.data();
        W.cap = L.total;
        L.stage(W.host);
    }
    // what the round trip does with no device: inputs over, results back
    void round_trip(const StageLayout &L) {
        memcpy(W.dev, W.host, L.in_bytes);
        if (L.out_bytes()) memcpy(W.host + L.out_begin, W.dev + L.out_begin, L.out_bytes());
        L.hand_over(W.host);
    }
};

template <class T>
void fill(T *p, size_t n, T first) {  // a kernel writing a whole slot
    for (size_t i = 0; i < n; ++i) p[i] = (T)(first + (T)i);
}

// mixed element sizes, zero-count slots, in / scratch / out interleaved by declaration order
void mixed_layout() {
    const auto a = iota<uint8_t>(3, 1);
    const auto b = iota<uint64_t>(33, 100);
    const auto c = iota<uint16_t>(129, 7);
    const std::vector<uint32_t> none;
    std::vector<uint32_t> r32(65, 0);
    std::vector<uint8_t> r8(257, 0);
    std::vector<double> r64(1, 0.0), untouched(4, -1.0);
    StageLayout L;
    const auto s_a = L.in(a.data(), a.size());
    const auto s_z = L.in(none.data(), 0);
    const auto s_b = L.in(b.data(), b.size());
    const auto s_h = L.in<uint32_t>(5);  // packed by hand
    const auto s_c = L.in(c.data(), c.size());
    L.end_inputs();
    const auto w_x = L.scratch<uint64_t>(9);
    const auto w_z = L.scratch<uint8_t>(0);
    const auto o_32 = L.out(r32.data(), r32.size());
    const auto o_z = L.out(untouched.data(), 0);
    const auto o_cut = L.out<uint16_t>(3);  // cut by hand
    const auto o_8 = L.out(r8.data(), r8.size());
    const auto o_no = L.out((double *)nullptr, 2);  // not asked for: a slot, no hand-over
    const auto o_64 = L.out(r64.data(), r64.size());
    expect(s_a.off == 0 && s_z.off == 256 && s_b.off == 256 && s_h.off == 768 && s_c.off == 1024, "input slots are 256-byte aligned, an empty one takes no room");
    expect(L.in_bytes == 1536 && w_x.off == 1536 && w_z.off == 1792, "the inputs end where the scratch begins");
    expect(L.out_begin == 1792 && o_32.off == 1792 && o_z.off == o_cut.off && o_z.count == 0, "the results begin behind the scratch");
    expect(L.total == o_64.off + 256 && L.out_bytes() == L.total - L.out_begin, "the last slot ends the layout");
    Blocks B(L);
    expect(!memcmp(B.W.host_ptr(s_a), a.data(), a.size()) && !memcmp(B.W.host_ptr(s_b), b.data(), 8 * b.size()) && !memcmp(B.W.host_ptr(s_c), c.data(), 2 * c.size()),
           "stage() copies every recorded input");
    fill(B.W.host_ptr(s_h), s_h.count, 40u);
    memcpy(B.W.dev, B.W.host, L.in_bytes);
    fill(B.W.dev_ptr(w_x), w_x.count, (uint64_t)1);
    fill(B.W.dev_ptr(o_32), o_32.count, 1000u);
    fill(B.W.dev_ptr(o_cut), o_cut.count, (uint16_t)50);
    fill(B.W.dev_ptr(o_8), o_8.count, (uint8_t)3);
    fill(B.W.dev_ptr(o_no), o_no.count, 0.5);
    fill(B.W.dev_ptr(o_64), o_64.count, 2.5);
    expect(B.W.dev_ptr_or_null(o_z) == nullptr && B.W.dev_ptr_or_null(o_32) == B.W.dev_ptr(o_32), "dev_ptr_or_null is null for an empty slot only");
    B.round_trip(L);
    expect(r32 == iota<uint32_t>(65, 1000) && r8 == iota<uint8_t>(257, 3) && r64[0] == 2.5, "hand_over() copies every recorded result");
    expect(untouched == std::vector<double>(4, -1.0), "a zero-count result is not touched");
    expect(B.W.host_ptr(o_cut)[2] == 52 && B.W.host_ptr(s_h)[4] == 44, "by-hand slots are the caller's to read and fill");
}

// a layout with no output: nothing comes back, nothing is handed over
void no_output() {
    const auto a = iota<uint32_t>(70, 0);
    StageLayout L;
    const auto s_a = L.in(a.data(), a.size());
    L.end_inputs();
    const auto w = L.scratch<uint32_t>(3);
    expect(L.out_bytes() == 0 && L.in_bytes == 512 && L.total == 768 && w.off == 512, "no output declared: out_bytes() is 0");
    Blocks B(L);
    B.round_trip(L);
    expect(!memcmp(B.W.dev_ptr(s_a), a.data(), 4 * a.size()), "the inputs reach the device block");
    StageLayout E;  // and one with outputs of no elements
    E.end_inputs();
    (void)E.out<uint32_t>(0);
    expect(E.out_bytes() == 0 && E.total == 0, "empty outputs: out_bytes() is 0");
}

// out_or_scratch: the array goes into L with its hand-over for a pointer, into D for NULL; dev_ptr follows it
void wanted_or_scratch() {
    std::vector<uint32_t> given(40, 0);
    std::vector<uint16_t> by_hand(6, 9);
    StageLayout L, D;
    L.end_inputs();
    (void)D.scratch<uint64_t>(5);
    const auto o_g = out_or_scratch(L, D, given.data(), given.size());
    const auto o_n = out_or_scratch(L, D, (double *)nullptr, 31);
    const auto o_h = out_or_scratch(L, D, by_hand.data(), by_hand.size(), /*by_hand=*/true);
    const auto o_m = out_or_scratch(L, D, (uint8_t *)nullptr, 1);
    expect(o_g.staged && !o_n.staged && o_h.staged && !o_m.staged, "staged exactly when the caller gave a pointer");
    expect(o_g.slot.off == 0 && o_h.slot.off == 256 && L.total == 512, "the wanted arrays lie in L in order");
    expect(o_n.slot.off == 256 && o_m.slot.off == 512 && D.total == 768, "the others lie in D behind its scratch");
    Blocks B(L);
    std::vector<char> ws_block(D.total, 0x77);
    DeviceScratch ws;
    ws.dev = ws_block.data();
    ws.cap = D.total;
    expect((char *)o_g.dev_ptr(B.W, ws) == B.W.dev && (char *)o_n.dev_ptr(B.W, ws) == ws.dev + 256, "dev_ptr comes from the buffer that holds the array");
    fill(o_g.dev_ptr(B.W, ws), o_g.slot.count, 5u);
    fill(o_n.dev_ptr(B.W, ws), o_n.slot.count, 1.0);
    fill(o_h.dev_ptr(B.W, ws), o_h.slot.count, (uint16_t)20);
    fill(o_m.dev_ptr(B.W, ws), o_m.slot.count, (uint8_t)1);
    B.round_trip(L);
    expect(given == iota<uint32_t>(40, 5), "a wanted array is handed over");
    expect(by_hand == std::vector<uint16_t>(6, 9) && B.W.host_ptr(o_h.slot)[5] == 25, "a by-hand array comes back to the mirror only");
}

// no device: a non-empty workspace fails with PHMM_ERR_HIP and stays empty, an empty one is granted without an allocation
void scratch_without_device() {
    phmm_handle h;
    DeviceScratch ws;
    StageLayout empty, D;
    (void)empty.scratch<uint32_t>(0);
    expect(ws.reserve(&h, empty, "check workspace") && !ws.dev && !ws.cap && h.err_code == PHMM_OK, "an empty layout reserves nothing");
    (void)D.scratch<uint32_t>(100);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) {
        expect(ws.reserve(&h, D, "check workspace") && ws.dev && ws.cap == D.total + D.total / 2, "with a device: 1.5x the need, no floor");
        ws.release();
    } else {
        expect(!ws.reserve(&h, D, "check workspace"), "no device: reserve fails");
        expect(h.err_code == PHMM_ERR_HIP && h.err.find("hipMalloc(check workspace)") != std::string::npos, "... with PHMM_ERR_HIP and the owner in the message");
    }
    expect(!ws.dev && !ws.cap, "... and the workspace stays empty");
    ws.release();
}

}  // namespace

int main() {
    mixed_layout();
    no_output();
    wanted_or_scratch();
    scratch_without_device();
    printf(failures ? "%d check(s) failed\n" : "staging_host_check: ok\n", failures);
    return failures != 0;
}

#include "engine_lanes.h"
#include "hash_batch.h"

// ------------------------------------------------------------------------------------------------------------
// SHA-256 of one message per lane (hash_batch.h): plain, double and tagged digests, and BIP-340 with a length per item
// ------------------------------------------------------------------------------------------------------------
// What every verifier of this engine takes as its 32-byte message is a digest of a preimage of a few hundred bytes.  These calls make
// the digests where the verifiers read them: one message per lane, 256 lanes per block, the blocks of a message one after the other
// (SHA-256 is serial within a message: nothing is shared across lanes).  A wavefront runs as many rounds as its longest message; items
// are not reordered by length (DESIGN.md 7.11 has the measured cost).
// MODE 0: SHA256(m); 1: SHA256(SHA256(m)); 2: the state behind the 64-byte tag prefix, then m (secp256k1_tagged_sha256).
template <int MODE>
__global__ void __launch_bounds__(256)
k_hash_batch(unsigned char* __restrict__ out32, hash_state start, const unsigned char* __restrict__ msgs, const u64* __restrict__ msg_off, u64 msglen, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    hash_batch_item<MODE == 2 ? 64 : 0, MODE == 1>(out32, start, msgs, msg_off, msglen, i);
}
// BIP-340 with the lane's own message pointer and length: schnorr_verify_lane as k_schnorr_verify (engine_core.hip) calls it
__global__ void __launch_bounds__(256, 2)
k_schnorr_verify_var(int32_t* __restrict__ results, schnorr_midstate mid, const unsigned char* __restrict__ sigs, const unsigned char* __restrict__ msgs,
                     const u64* __restrict__ msg_off, const unsigned char* __restrict__ pks, int pk_format, const u32* __restrict__ gtab, u32* __restrict__ ptab, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int live = i < n;
    const size_t ii = live ? i : 0;
    __shared__ u32 s_dig[S2K_DIG_WORDS * 256];
    const lane_mem lm{ptab + i * S2K_PTAB_WORDS, S2K_LANE_DIG(s_dig)};
    u64 at, len;
    const int span = hash_item_span(at, len, msg_off, 0, ii);          // (a decreasing pair: no message byte is read, the verdict is 0)
    const int r = schnorr_verify_lane(mid, sigs + 64 * ii, msgs + at, (size_t)len, pks + (pk_format ? 64 : 32) * ii, pk_format, live & span, gtab, lm);
    if (live) results[i] = r;
}

// ---- the host's share: a tag's midstate (host_sha256.h) ------------------------------------------------------------------------------------
static void host_sha256_words(uint32_t s[8], const unsigned char* p, size_t len) {
    static const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    memcpy(s, iv, sizeof(iv));
    size_t rem = len;
    for (; rem >= 64; p += 64, rem -= 64) host_sha256_compress(s, p);
    unsigned char blk[128] = {0};
    if (rem) memcpy(blk, p, rem);
    blk[rem] = 0x80;
    const size_t end = rem < 56 ? 64 : 128;
    const uint64_t bits = (uint64_t)len << 3;
    for (int k = 0; k < 8; k++) blk[end - 1 - k] = (unsigned char)(bits >> (8 * k));
    host_sha256_compress(s, blk);
    if (end == 128) host_sha256_compress(s, blk + 64);
}
// the state behind SHA256(tag) | SHA256(tag): secp256k1_sha256_initialize_tagged (src/hash_impl.h)
static hash_state tag_midstate(const unsigned char* tag, size_t taglen) {
    uint32_t th[8];
    host_sha256_words(th, tag, taglen);
    unsigned char blk[64];
    for (int i = 0; i < 8; i++) { s2k_store_be32(blk + 4 * i, th[i]); s2k_store_be32(blk + 32 + 4 * i, th[i]); }
    hash_state m;
    sha256_init(m.s);
    host_sha256_compress(m.s, blk);
    return m;
}
static hash_state plain_start() { hash_state m; sha256_init(m.s); return m; }

// ---- digests ----------------------------------------------------------------------------------------------------------------------------------
// mode: 0 plain, 1 double, 2 tagged (start: the tag's midstate)
static int hash_dev(s2k_engine* e, void* stream, unsigned char* out32, int mode, const hash_state& start, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen,
                    size_t n) {
    return lanes_run(e, stream, n, {false, false, 0}, {{out32, 32 * n}}, [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        unsigned char* o = out32 + 32 * i0;
        const unsigned char* p = msg_off ? msgs : msgs + msglen * i0;
        const u64* off = msg_off ? (const u64*)msg_off + i0 : nullptr;
        if (mode == 0) hipLaunchKernelGGL(k_hash_batch<0>, grid, dim3(256), 0, st, o, start, p, off, (u64)msglen, m);
        else if (mode == 1) hipLaunchKernelGGL(k_hash_batch<1>, grid, dim3(256), 0, st, o, start, p, off, (u64)msglen, m);
        else hipLaunchKernelGGL(k_hash_batch<2>, grid, dim3(256), 0, st, o, start, p, off, (u64)msglen, m);
    });
}
// the bytes [msg_off[0], msg_off[n]) and offsets relative to their start (der_window's rule); the fixed-length form: n * msglen bytes
struct msg_span { const unsigned char* lo; size_t bytes; std::vector<uint64_t> rel; };
static int msg_window(const char* who, msg_span& w, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen, size_t n) {
    w.lo = msgs; w.bytes = msglen * n;
    if (!msg_off) return 1;
    for (size_t i = 0; i < n; i++) if (msg_off[i + 1] < msg_off[i]) return s2k_fail_arg(who, "msg_off must not decrease");
    w.lo = msgs + msg_off[0]; w.bytes = (size_t)(msg_off[n] - msg_off[0]);
    w.rel.resize(n + 1);
    for (size_t i = 0; i <= n; i++) w.rel[i] = msg_off[i] - msg_off[0];
    return 1;
}
static int hash_host(const char* who, s2k_engine* e, unsigned char* out32, int mode, const hash_state& start, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen,
                     size_t n) {
    msg_span mw;
    if (!msg_window(who, mw, msgs, msg_off, msglen, n)) return 0;
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    stage_buf b[] = {{nullptr, out32, 32 * n}, {mw.lo, nullptr, mw.bytes}, {msg_off ? mw.rel.data() : nullptr, nullptr, 8 * (n + 1)}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, hash_dev(e, nullptr, b[0].at(), mode, start, b[1].at(), b[2].opt<uint64_t>(), msglen, n));
}

extern "C" int s2k_sha256_batch_dev(s2k_engine* e, void* stream, unsigned char* out32, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen, int rounds, size_t n) {
    const char* who = "s2k_sha256_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out32 || !msgs) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (rounds != 1 && rounds != 2) return s2k_fail_arg(who, "rounds must be 1 (SHA256) or 2 (SHA256 of SHA256)");
    return hash_dev(e, stream, out32, rounds - 1, plain_start(), msgs, msg_off, msglen, n);
}
extern "C" int s2k_sha256_batch(s2k_engine* e, unsigned char* out32, const unsigned char* msgs, const uint64_t* msg_off, size_t msglen, int rounds, size_t n) {
    const char* who = "s2k_sha256_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out32 || !msgs) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    if (rounds != 1 && rounds != 2) return s2k_fail_arg(who, "rounds must be 1 (SHA256) or 2 (SHA256 of SHA256)");
    return hash_host(who, e, out32, rounds - 1, plain_start(), msgs, msg_off, msglen, n);
}
extern "C" int secp256k1_tagged_sha256_batch_dev(s2k_engine* e, void* stream, unsigned char* out32, const unsigned char* tag, size_t taglen, const unsigned char* msgs,
                                                 const uint64_t* msg_off, size_t msglen, size_t n) {
    const char* who = "secp256k1_tagged_sha256_batch_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out32 || !tag || !msgs) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return hash_dev(e, stream, out32, 2, tag_midstate(tag, taglen), msgs, msg_off, msglen, n);
}
extern "C" int secp256k1_tagged_sha256_batch(s2k_engine* e, unsigned char* out32, const unsigned char* tag, size_t taglen, const unsigned char* msgs, const uint64_t* msg_off,
                                             size_t msglen, size_t n) {
    const char* who = "secp256k1_tagged_sha256_batch";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!out32 || !tag || !msgs) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    return hash_host(who, e, out32, 2, tag_midstate(tag, taglen), msgs, msg_off, msglen, n);
}

// ---- BIP-340, a message length per item ---------------------------------------------------------------------------------------------------------
extern "C" int secp256k1_schnorrsig_verify_batch_var_dev(s2k_engine* e, void* stream, int32_t* results, const unsigned char* sigs, const unsigned char* msgs,
                                                         const uint64_t* msg_off, const unsigned char* pubkeys, int pk_format, size_t n) {
    const char* who = "secp256k1_schnorrsig_verify_batch_var_dev";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msgs || !msg_off || !pubkeys) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    const size_t pkb = pk_format ? 64 : 32;
    return lanes_run(e, stream, n, {true, true, 0}, {{results, sizeof(int32_t) * n}},         // a batch that does not complete never shows an item as valid
                     [&](size_t i0, size_t m, dim3 grid, hipStream_t st, u32*) {
        hipLaunchKernelGGL(k_schnorr_verify_var, grid, dim3(256), 0, st, results + i0, e->bip340, sigs + 64 * i0, msgs, (const u64*)msg_off + i0, pubkeys + pkb * i0, pk_format,
                           e->gtab, e->ptab, m);
    });
}
extern "C" int secp256k1_schnorrsig_verify_batch_var(s2k_engine* e, int32_t* results, const unsigned char* sigs, const unsigned char* msgs, const uint64_t* msg_off,
                                                     const unsigned char* pubkeys, int pk_format, size_t n) {
    const char* who = "secp256k1_schnorrsig_verify_batch_var";
    if (!e) return s2k_fail(who, "null engine");
    if (n == 0) return 1;
    if (!results || !sigs || !msgs || !msg_off || !pubkeys) return s2k_fail_arg(who, "illegal argument (ARG_CHECK)");
    msg_span mw;
    if (!msg_window(who, mw, msgs, msg_off, 0, n)) return 0;
    memset(results, 0, sizeof(int32_t) * n);
    std::lock_guard<std::recursive_mutex> lock(e->mu);
    HIPCHK(hipSetDevice(e->device));
    const size_t pkb = pk_format ? 64 : 32;
    stage_buf b[] = {{nullptr, results, 4 * n}, {sigs, nullptr, 64 * n}, {mw.lo, nullptr, mw.bytes}, {mw.rel.data(), nullptr, 8 * (n + 1)}, {pubkeys, nullptr, pkb * n}};
    if (!stage_open(e, b)) return 0;
    return stage_close(e, b, secp256k1_schnorrsig_verify_batch_var_dev(e, nullptr, b[0].at<int32_t>(), b[1].at(), b[2].at(), b[3].at<uint64_t>(), b[4].at(), pk_format, n));
}

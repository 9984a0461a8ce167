// qshare_packed_check.cpp -- the host restatement of the packed-round queue of the shadow-fed shared-row
// scan (weaviate_amd/csrc/wvg_qshare.hip, "Packed rounds"): a wave appends each tile's admitted (row,
// query) pairs to a queue of 32-bit entries, runs a round of 64 from the top while 64 are pending, and
// empties the queue after the last tile of its range, after the last tile of every block of 2^IBITS tile
// positions (an entry holds the position modulo 2^IBITS) and after a tile that admitted LOOSE pairs or more.
//
// main() drives the queue with random and extreme admission masks and checks that every pair comes out
// exactly once with its own (tile, row, query), that the count never exceeds the capacity, and that the
// queue is empty at the end of a pass.  Stand-alone, no GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/qshare_packed_check.cpp -o qshare_packed_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

namespace {

constexpr int CAP = 63 + 16 * 64;  // QSP_CAP
constexpr int LOOSE = 8;           // QSP_LOOSE

struct Queue {
    int ibits;
    uint64_t imask;
    std::vector<uint32_t> pend = std::vector<uint32_t>(CAP);  // ASan guards both ends
    uint32_t n = 0, high = 0;
    uint64_t rounds = 0, loose_tiles = 0;
    std::multiset<uint64_t> out;  // (tile position, row, query) of every popped entry

    explicit Queue(int ib) : ibits(ib), imask((1ull << ib) - 1) {}

    // adm[lane] = the lane's 16 admission bits (bit 4 rg + r: row 16 rg + (lane & 15), query 4 (lane >> 4) + r)
    void append(uint64_t i, const uint32_t (&adm)[64])
    {
        for (int rg = 0; rg < 4; rg++)
            for (int r = 0; r < 4; r++) {
                uint32_t rank = 0;  // the ballot's prefix popcount
                for (int lane = 0; lane < 64; lane++) {
                    if (!((adm[lane] >> (4 * rg + r)) & 1u)) continue;
                    const uint32_t ent = (uint32_t)(i & imask) << 10 | (uint32_t)(lane & 15) << 4 | (uint32_t)(lane >> 4) * 4;
                    if (n + rank >= (uint32_t)CAP) {
                        std::printf("FAIL: overflow at tile %llu\n", (unsigned long long)i);
                        std::exit(1);
                    }
                    pend[n + rank] = ent + (uint32_t)(rg << 8 | r);
                    rank++;
                }
                n += rank;
            }
        high = n > high ? n : high;
    }

    void drain(uint64_t i, uint64_t ntiles, uint32_t n0)
    {
        const bool flush = i + 1 == ntiles || ((i + 1) & imask) == 0 || n - n0 >= (uint32_t)LOOSE;
        loose_tiles += n - n0 >= (uint32_t)LOOSE;
        const uint64_t iblock = i & ~imask;
        while (n >= 64 || (flush && n != 0)) {
            rounds++;
            const uint32_t take = n < 64 ? n : 64;
            n -= take;
            for (uint32_t lane = 0; lane < take; lane++) {
                const uint32_t e = pend[n + lane];
                out.insert((iblock + (e >> 10)) << 10 | (e & 1023u));
            }
        }
    }
};

int run(int ibits, uint64_t ntiles, int kind, uint32_t seed)
{
    std::mt19937 rng(seed);
    Queue q(ibits);
    std::multiset<uint64_t> want;
    uint64_t pairs = 0;
    for (uint64_t i = 0; i < ntiles; i++) {
        uint32_t adm[64];
        for (int lane = 0; lane < 64; lane++) {
            uint32_t a = 0;
            switch (kind) {
            case 0: a = rng() % 97 == 0 ? 1u << (rng() % 16) : 0u; break;          // sparse: the bench's ~3 per tile
            case 1: a = 0xFFFFu; break;                                          // every pair of every tile
            case 2: a = i % 3 == 1 ? 0u : (rng() & rng() & 0xFFFFu); break;       // dense, with empty tiles
            case 3: a = i + 1 == ntiles ? 0u : (lane == 5 ? 0x0001u : 0u); break;  // one pair a tile, empty last tile
            case 4: a = (rng() % 8 == 0) ? 0x1111u << (rng() % 4) : 0u; break;    // one open query per group
            default: a = i % 2 == 0 ? (lane < 63 ? 1u : 0u) : 0xFFFFu; break;      // 63 pending, then a full tile: CAP
            }
            adm[lane] = a;
            for (int b = 0; b < 16; b++)
                if ((a >> b) & 1u) {
                    want.insert(i << 10 | (uint64_t)((b >> 2) * 16 + (lane & 15)) << 4 | (uint64_t)((lane >> 4) * 4 + (b & 3)));
                    pairs++;
                }
        }
        const uint32_t n0 = q.n;
        q.append(i, adm);
        q.drain(i, ntiles, n0);
        if (q.n >= 64) {
            std::printf("FAIL: %u pending after tile %llu\n", q.n, (unsigned long long)i);
            return 1;
        }
    }
    const uint64_t blocks = (ntiles + q.imask) >> ibits;
    if (q.n != 0 || q.out != want || q.high > (uint32_t)CAP || q.rounds > pairs / 64 + blocks + q.loose_tiles) {
        std::printf("FAIL: ibits %d tiles %llu kind %d: left %u, out %zu want %zu, high %u, rounds %llu\n", ibits,
                    (unsigned long long)ntiles, kind, q.n, q.out.size(), want.size(), q.high, (unsigned long long)q.rounds);
        return 1;
    }
    std::printf("ok: ibits %2d tiles %4llu kind %d: %7llu pairs in %6llu rounds, at most %4u pending\n", ibits,
                (unsigned long long)ntiles, kind, (unsigned long long)pairs, (unsigned long long)q.rounds, q.high);
    return 0;
}

}  // namespace

int main()
{
    int bad = 0;
    uint32_t seed = 1;
    for (int ibits : {22, 3})  // 3: ranges that cross several blocks of tile positions
        for (uint64_t ntiles : {1ull, 2ull, 7ull, 8ull, 9ull, 61ull, 300ull})
            for (int kind = 0; kind < 6; kind++) bad += run(ibits, ntiles, kind, seed++);
    if (bad) return 1;
    std::printf("all ok\n");
    return 0;
}

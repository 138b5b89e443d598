// Stand-alone run of csrc/rifraf_seq_upload.h for the host sanitizers: the
// coding passes on 1 and on 4 threads, a full dictionary, the undo and the
// chunk splitter, on inputs of the shapes tests/test_seq_upload_host.py uses.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tests/host/seq_upload_main.cpp -o seq_upload_main && ./seq_upload_main
//
// Exit status 0 and "seq_upload_main: ok" when every check holds.
#include <cstdio>
#include <random>

#include "../../rifraf.jl_amd/csrc/rifraf_seq_upload.h"

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

struct Tables {
    std::vector<uint8_t> bases;
    std::vector<int64_t> off{0};
    std::vector<double> match, mismatch, ins, del;
    template <class Draw>
    void add(int64_t n, Draw draw)
    {
        for (int64_t i = 0; i < n; ++i) {
            bases.push_back((uint8_t)(i & 3));
            match.push_back(draw());
            mismatch.push_back(draw());
            ins.push_back(draw());
        }
        for (int64_t i = 0; i <= n; ++i)
            del.push_back(draw());
        off.push_back(off.back() + n);
    }
};

struct Result {
    std::vector<uint8_t> coded, finite;
    std::vector<uint64_t> rec;
    std::vector<double> v3 = std::vector<double>((size_t)RF_CODES * 4), v1 = std::vector<double>(RF_CODES);
    int64_t sizes[3] = {};
};

static int run(const Tables &t, const std::vector<int32_t> &up, const std::vector<uint8_t> &flags, int nth, Result &r)
{
    const int32_t nseq = (int32_t)t.off.size() - 1;
    r.coded.assign(nseq, 0);
    r.finite.assign(nseq, 0);
    r.rec.assign(t.off.back(), 0);
    return host_row_codes(nseq, t.bases.data(), t.off.data(), t.match.data(), t.mismatch.data(), t.ins.data(),
                          t.del.data(), (int32_t)up.size() - 1, up.data(), flags.data(), nth, r.coded.data(),
                          r.finite.data(), r.rec.data(), r.v3.data(), r.v1.data(), r.sizes);
}

int main()
{
    std::mt19937_64 g(1212);
    std::vector<double> pool{-__builtin_inf(), -0.0, 0.0};
    for (int k = 1; k < 28; ++k)
        pool.push_back(-0.25 * k);
    auto draw = [&] { return pool[g() % pool.size()]; };
    // 12 sequences of 1..40 positions over the pool: 1 thread and 4 agree
    Tables t;
    for (int64_t n : {1, 40, 7, 13, 22, 3, 31, 38, 2, 17, 9, 26})
        t.add(n, draw);
    Result a, b;
    CHECK(run(t, {0, 12}, {0}, 1, a) == 0 && run(t, {0, 12}, {0}, 4, b) == 0);
    CHECK(a.rec == b.rec && a.coded == b.coded && a.finite == b.finite);
    CHECK(a.sizes[0] == b.sizes[0] && a.sizes[1] == b.sizes[1] && a.sizes[2] == 0);
    CHECK(std::memcmp(a.v3.data(), b.v3.data(), a.sizes[0] * 32) == 0);
    CHECK(std::memcmp(a.v1.data(), b.v1.data(), a.sizes[1] * 8) == 0);
    // undo: [A][B undone][C] codes C as [A][C] does
    Tables ac = t, abc = t;
    std::mt19937_64 g2 = g;
    for (int64_t n : {12, 3, 8})
        abc.add(n, [&] { return draw() - 100.0; });
    g = g2;
    ac.add(10, draw);
    g = g2;
    abc.add(10, draw);
    Result c, d;
    CHECK(run(ac, {0, 12, 13}, {0, 0}, 2, c) == 0 && run(abc, {0, 12, 15, 16}, {0, 2, 0}, 2, d) == 0);
    CHECK(c.sizes[0] == d.sizes[0] && c.sizes[1] == d.sizes[1]);
    CHECK(std::memcmp(c.v3.data(), d.v3.data(), c.sizes[0] * 32) == 0);
    CHECK(std::equal(c.rec.end() - 10, c.rec.end(), d.rec.end() - 10));
    // a full dictionary: 67 x 1000 distinct triples, then a held sequence, then a fresh upload
    Tables big;
    double x = -1.0;
    for (int k = 0; k < 67; ++k) {
        int i = 0;
        big.add(1000, [&] { return (i++ % 3 == 0 && i <= 3000) ? (x -= 1e-6) : -3.0; });
    }
    Result f;
    CHECK(run(big, {0, 67}, {0}, 4, f) == 0);
    CHECK(f.sizes[0] == RF_CODES && f.sizes[2] == 2 && f.coded[64] == 1 && f.coded[65] == 0);
    Tables more = big;
    int i = 0;
    more.add(1000, [&] { return (i++ % 3 == 0 && i <= 3000) ? big.match[(i - 1) / 3] : -3.0; });
    more.add(5, draw);
    CHECK(run(more, {0, 67, 68, 69}, {0, 0, 1}, 3, f) == 0);
    CHECK(f.coded[67] == 1 && f.coded[68] == 1 && f.sizes[0] <= 5 && f.sizes[2] == 2);
    // the splitter: [5, 5, 5, 100, 1, 1] at, below and above every boundary
    const std::vector<int64_t> off{0, 5, 10, 15, 115, 116, 117};
    std::vector<int32_t> end(6);
    int32_t nc = 0;
    for (int codes = 0; codes < 2; ++codes)
        for (int64_t budget = 1; budget < 5000; ++budget) {
            CHECK(host_upload_chunks(6, off.data(), nullptr, nullptr, codes, 0, budget, end.data(), &nc) == 0);
            CHECK(nc >= 1 && nc <= 6 && end[nc - 1] == 6);
        }
    for (int stage_kb : {16, 262144}) {
        CHECK(host_upload_chunks(6, off.data(), nullptr, nullptr, 0, stage_kb, 0, end.data(), &nc) == 0 && nc == 1);
        CHECK(host_upload_chunks(6, off.data(), nullptr, nullptr, 1, stage_kb, 0, end.data(), &nc) == 0 && nc == 1);
    }
    std::printf("seq_upload_main: ok\n");
    return 0;
}

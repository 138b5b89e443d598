// rifraf_seq_upload.h -- the host side of the sequence uploads
// (rf_set_sequences, rf_set_sequences_codes) that touches no device: the
// length of a sequence's table region, the row codes' dictionary, the three
// coding passes and the chunk splitter.  No HIP: a plain C++17 compiler takes
// it alone.  The steps are stated once in DESIGN.md §4 "Sequence uploads".
#ifndef RIFRAF_SEQ_UPLOAD_H
#define RIFRAF_SEQ_UPLOAD_H

#include <cmath>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <utility>

#include "rifraf_dp_plan.h"

constexpr int RF_CODES = 1 << 16;   // entries of the row codes' dictionary (DPTask: rifraf_dp_plan.h)
// A sequence's table region: [match|mismatch|ins|del|cins|cdel], then one
// row-code record per position.  Doubles from its start to the records, and
// its length in doubles.
RF_HD inline int64_t row_code_off(int64_t n, int64_t nci, int64_t ncd) { return 4 * n + 1 + nci + ncd; }
RF_HD inline int64_t seq_table_len(int64_t n, int64_t nci, int64_t ncd) { return row_code_off(n, nci, ncd) + n; }

template <class F>
void parallel_for(int nth, F fn)
{
    if (nth <= 1) {
        fn(0);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 1; t < nth; ++t)
        th.emplace_back(fn, t);
    fn(0);
    for (auto &x : th)
        x.join();
}

// Code dictionary of the row codes (RF_TASK_CODED): every distinct
// (match, mismatch, ins) triple and del value of the context's reads gets a
// 16-bit code, first come first served, keyed by the exact bit patterns.  A
// read whose values would need a code past RF_CODES - 1 stays uncoded (its
// DP reads the tables directly; counted in `uncoded_reads`, rf_code_stats).
// Entries are only appended while any coded sequence outside an upload is
// still valid, so codes of earlier reads stay valid; an upload that replaces
// every coded sequence of the context starts a fresh dictionary, so a
// long-lived context refilled batch after batch does not fill it up.  The
// device copies (RF_CODES x 4 triple doubles, then RF_CODES del doubles; the
// off-base values) belong to the context.
struct CodeDict {
    struct K3 {
        uint64_t a, b, c;
        bool operator==(const K3 &o) const { return a == o.a && b == o.b && c == o.c; }
    };
    struct H3 {
        size_t operator()(const K3 &k) const
        {
            return (size_t)((k.a * 0x9E3779B97F4A7C15ull) ^ (k.b * 0xC2B2AE3D27D4EB4Full) ^ (k.c * 0x165667B19E3779F9ull));
        }
    };
    std::unordered_map<K3, uint32_t, H3> t3;
    std::unordered_map<uint64_t, uint32_t> d1;
    std::vector<double> t3v, d1v;   // host copies of the entries: {match, mismatch, ins, 0} per triple; del
    size_t up3 = 0, up1 = 0;        // entries already on the device
    int64_t uncoded_reads = 0;      // reads left uncoded because the dictionary was full
    int64_t resets = 0;
    // per triple entry: log10(1 - 10^match) - log10(3), the off-base value of
    // base_distribution (model.jl:804-809), host libm
    std::vector<double> errv;
    size_t uperr = 0;               // of these, already on the device

    void reset()
    {
        t3.clear();
        d1.clear();
        t3v.clear();
        d1v.clear();
        errv.clear();
        up3 = up1 = uperr = 0;
        ++resets;
    }

    static uint64_t bits(double x)
    {
        uint64_t u;
        std::memcpy(&u, &x, 8);
        return u;
    }
    static double value(uint64_t u)
    {
        double x;
        std::memcpy(&x, &u, 8);
        return x;
    }
    static K3 key3(double match, double mismatch, double ins) { return {bits(match), bits(mismatch), bits(ins)}; }
    // read-only lookups (safe from several threads while nothing is inserted)
    int32_t find3(const K3 &k) const
    {
        auto it = t3.find(k);
        return it == t3.end() ? -1 : (int32_t)it->second;
    }
    int32_t find1(uint64_t k) const
    {
        auto it = d1.find(k);
        return it == d1.end() ? -1 : (int32_t)it->second;
    }
    // The code of a triple / del value, a new one if it has none: -1 when
    // RF_CODES are held.  Codes count up from 0 in insertion order.
    int32_t insert3(const K3 &k)
    {
        const int32_t c = find3(k);
        if (c >= 0 || t3.size() >= (size_t)RF_CODES)
            return c;
        const uint32_t id = (uint32_t)t3.size();
        t3.emplace(k, id);
        t3v.insert(t3v.end(), {value(k.a), value(k.b), value(k.c), 0.0});
        return (int32_t)id;
    }
    int32_t insert1(uint64_t k)
    {
        const int32_t c = find1(k);
        if (c >= 0 || d1.size() >= (size_t)RF_CODES)
            return c;
        const uint32_t id = (uint32_t)d1.size();
        d1.emplace(k, id);
        d1v.push_back(value(k));
        return (int32_t)id;
    }
    // undo(mark()) drops the entries inserted in between: the maps, t3v / d1v
    // and the code the next insert takes are as they were at the mark.
    struct Mark {
        size_t n3, n1;
    };
    Mark mark() const { return {t3.size(), d1.size()}; }
    void undo(const Mark &m)
    {
        for (size_t e = m.n3; 4 * e < t3v.size(); ++e)
            t3.erase(key3(t3v[4 * e], t3v[4 * e + 1], t3v[4 * e + 2]));
        for (size_t e = m.n1; e < d1v.size(); ++e)
            d1.erase(bits(d1v[e]));
        t3v.resize(4 * m.n3);
        d1v.resize(m.n1);
        errv.resize(std::min(errv.size(), m.n3));
        up3 = std::min(up3, m.n3);
        up1 = std::min(up1, m.n1);
        uperr = std::min(uperr, m.n3);
    }
    // per-thread direct-mapped front cache of the lookups (a read set has few
    // distinct values; misses fall through to the maps)
    struct Cache {
        std::vector<std::pair<K3, int32_t>> c3 = std::vector<std::pair<K3, int32_t>>(1024, {K3{}, -2});
        std::vector<std::pair<uint64_t, int32_t>> c1 = std::vector<std::pair<uint64_t, int32_t>>(1024, {0, -2});
    };
    int32_t find3(const K3 &k, Cache &C) const
    {
        auto &e = C.c3[(H3()(k) >> 32) & 1023];
        if (e.second != -2 && e.first == k)
            return e.second;
        const int32_t v = find3(k);
        if (v >= 0)
            e = {k, v};
        return v;
    }
    int32_t find1(uint64_t k, Cache &C) const
    {
        auto &e = C.c1[((k * 0x9E3779B97F4A7C15ull) >> 40) & 1023];
        if (e.second != -2 && e.first == k)
            return e.second;
        const int32_t v = find1(k);
        if (v >= 0)
            e = {k, v};
        return v;
    }
};

// One sequence of a tables upload: `tab` is its table region in host memory
// (seq_table_len doubles), the caller's tables packed by pack_tables; the
// coding passes write its records behind the tables and the two flags.
struct RowSeq {
    double *tab;
    const uint8_t *bases;
    int64_t n, nci, ncd;
    bool finite;   // no non-finite entry among match / mismatch / ins / del (4 n + 1 values)
    bool coded;    // every position has a record
};

// The caller's tables of one sequence (cins / cdel: nci / ncd entries, else unread) into its region
inline void pack_tables(const RowSeq &s, const double *match, const double *mismatch, const double *ins,
                        const double *del, const double *cins, const double *cdel)
{
    double *h = s.tab;
    const int64_t n = s.n;
    std::memcpy(h, match, n * 8);
    std::memcpy(h + n, mismatch, n * 8);
    std::memcpy(h + 2 * n, ins, n * 8);
    std::memcpy(h + 3 * n, del, (n + 1) * 8);
    if (s.nci)
        std::memcpy(h + 4 * n + 1, cins, s.nci * 8);
    if (s.ncd)
        std::memcpy(h + 4 * n + 1 + s.nci, cdel, s.ncd * 8);
}

// The row codes of the sequences seq[0, nseq) on nth threads, each over a
// range of sequences, in three passes so that one thread alone writes the
// dictionary: the new keys of every range (read-only lookups), their
// insertion in range order (= the serial first-occurrence order, whatever
// nth), then the records (read-only lookups).  pack(k) runs first on the
// thread that takes sequence k: it brings seq[k]'s tables into seq[k].tab
// (pack_tables; nothing to do when they lie there already).  A key that finds
// the dictionary full keeps its sequence uncoded; keys of that sequence that
// still fitted stay in the dictionary.
template <class Pack>
void code_rows(CodeDict &D, RowSeq *seq, int32_t nseq, int nth, Pack pack)
{
    nth = std::max(nth, 1);
    std::vector<int32_t> rng(nth + 1);
    for (int t = 0; t <= nth; ++t)
        rng[t] = (int32_t)((int64_t)nseq * t / nth);
    std::vector<std::vector<CodeDict::K3>> new3(nth);
    std::vector<std::vector<uint64_t>> new1(nth);
    parallel_for(nth, [&](int t) {
        std::unordered_set<CodeDict::K3, CodeDict::H3> s3;
        std::unordered_set<uint64_t> s1;
        CodeDict::Cache cache;
        for (int32_t k = rng[t]; k < rng[t + 1]; ++k) {
            pack(k);
            RowSeq &S = seq[k];
            const int64_t n = S.n;
            const double *h = S.tab;
            bool fin = true;
            for (int64_t e = 0; e < 4 * n + 1; ++e)
                fin = fin && std::isfinite(h[e]);
            S.finite = fin;
            for (int64_t i = 0; i < n; ++i) {
                const CodeDict::K3 key = CodeDict::key3(h[i], h[n + i], h[2 * n + i]);
                if (D.find3(key, cache) < 0 && s3.insert(key).second)
                    new3[t].push_back(key);
            }
            for (int64_t i = 0; i <= n; ++i) {
                const uint64_t key = CodeDict::bits(h[3 * n + i]);
                if (D.find1(key, cache) < 0 && s1.insert(key).second)
                    new1[t].push_back(key);
            }
        }
    });
    for (int t = 0; t < nth; ++t) {
        for (const auto &key : new3[t])
            D.insert3(key);
        for (uint64_t key : new1[t])
            D.insert1(key);
    }
    // a record: bits 0-15 the triple's code, 16-31 / 32-47 the codes of
    // del[i] / del[i + 1], 48-55 the base
    parallel_for(nth, [&](int t) {
        CodeDict::Cache cache;
        for (int32_t k = rng[t]; k < rng[t + 1]; ++k) {
            RowSeq &S = seq[k];
            const int64_t n = S.n;
            const double *h = S.tab;
            uint64_t *rec = (uint64_t *)(S.tab + row_code_off(n, S.nci, S.ncd));
            int32_t dprev = D.find1(CodeDict::bits(h[3 * n]), cache);
            bool ok = dprev >= 0;
            for (int64_t i = 0; i < n && ok; ++i) {
                const int32_t c3 = D.find3(CodeDict::key3(h[i], h[n + i], h[2 * n + i]), cache);
                const int32_t dn = D.find1(CodeDict::bits(h[3 * n + i + 1]), cache);
                ok = c3 >= 0 && dn >= 0;
                rec[i] = (uint64_t)(uint32_t)c3 | ((uint64_t)(uint32_t)dprev << 16) | ((uint64_t)(uint32_t)dn << 32) |
                         ((uint64_t)S.bases[i] << 48);
                dprev = dn;
            }
            S.coded = ok;
        }
    });
    for (int32_t k = 0; k < nseq; ++k)
        D.uncoded_reads += seq[k].coded ? 0 : 1;
}

// The uploads stage their sequences in chunks: the chunk from sequence k0
// takes k0, then further sequences while the chunk's bytes stay within the
// budget.  Returns one past its last sequence.  bytes(k): the staged bytes of
// sequence k.
template <class Bytes>
int32_t chunk_end(int32_t k0, int32_t nseq, int64_t budget, Bytes bytes)
{
    int64_t sum = bytes(k0);
    int32_t k1 = k0 + 1;
    for (; k1 < nseq && sum + bytes(k1) <= budget; ++k1)
        sum += bytes(k1);
    return k1;
}
// The two paths' staged bytes per sequence and their budgets at RF_OPT_STAGE_KB:
// rf_set_sequences stages 8 B per double of the table region,
// rf_set_sequences_codes a base and a code per position (a quarter of the
// option, at least 1 MB: its chunks cost a launch set each).
inline int64_t tables_stage_bytes(int64_t n, int64_t nci, int64_t ncd) { return seq_table_len(n, nci, ncd) * 8; }
inline int64_t tables_stage_budget(int stage_kb) { return (int64_t)std::max(stage_kb, 1) * 1024; }
inline int64_t codes_stage_bytes(int64_t n) { return 2 * n; }
inline int64_t codes_stage_budget(int stage_kb) { return std::max<int64_t>((int64_t)stage_kb * 1024 / 4, 1 << 20); }

// rf_host_row_codes (include/rifraf_hip.h): code_rows for the uploads
// [up[u], up[u + 1]) of nseq sequences without codon tables, on a dictionary
// of its own.  flags[u] & 1: the upload starts a fresh dictionary; & 2: its
// entries are undone after it (the codes path's refusal).
inline int host_row_codes(int32_t nseq, const uint8_t *bases, const int64_t *off, const double *match,
                          const double *mismatch, const double *ins, const double *del, int32_t nup,
                          const int32_t *up, const uint8_t *flags, int32_t nthreads, uint8_t *coded, uint8_t *finite,
                          uint64_t *records, double *val3, double *val1, int64_t *sizes)
{
    if (nseq < 0 || nup < 0 || nthreads < 1 || !sizes || (nup > 0 && (!up || !flags || up[0] != 0 || up[nup] != nseq)) ||
        (nup == 0 && nseq > 0) ||
        (nseq > 0 && (!bases || !off || !match || !mismatch || !ins || !del || !coded || !finite || !records || !val3 ||
                      !val1)))
        return RF_ERR_ARG;
    for (int32_t k = 0; k < nseq; ++k)
        if (off[k + 1] - off[k] < 1)
            return RF_ERR_ARG;
    for (int32_t u = 0; u < nup; ++u)
        if (up[u + 1] < up[u])
            return RF_ERR_ARG;
    CodeDict D;
    std::vector<double> stage;
    std::vector<RowSeq> rs;
    for (int32_t u = 0; u < nup; ++u) {
        const int32_t k0 = up[u], n = up[u + 1] - up[u];
        if (flags[u] & 1)
            D.reset();
        const CodeDict::Mark mark = D.mark();
        rs.resize(n);
        int64_t nt = 0;
        for (int32_t k = 0; k < n; ++k)
            nt += seq_table_len(off[k0 + k + 1] - off[k0 + k], 0, 0);
        stage.resize(nt);
        nt = 0;
        for (int32_t k = 0; k < n; ++k) {
            const int64_t len = off[k0 + k + 1] - off[k0 + k];
            rs[k] = {stage.data() + nt, bases + off[k0 + k], len, 0, 0, false, false};
            nt += seq_table_len(len, 0, 0);
        }
        code_rows(D, rs.data(), n, nthreads, [&](int32_t k) {
            const int32_t kg = k0 + k;
            pack_tables(rs[k], match + off[kg], mismatch + off[kg], ins + off[kg], del + off[kg] + kg, nullptr,
                        nullptr);
        });
        for (int32_t k = 0; k < n; ++k) {
            coded[k0 + k] = rs[k].coded;
            finite[k0 + k] = rs[k].finite;
            // an uncoded sequence's records are unspecified: zeros here
            uint64_t *out = records + (off[k0 + k] - off[0]);
            if (rs[k].coded)
                std::memcpy(out, rs[k].tab + row_code_off(rs[k].n, 0, 0), rs[k].n * 8);
            else
                std::fill(out, out + rs[k].n, (uint64_t)0);
        }
        if (flags[u] & 2)
            D.undo(mark);
    }
    if (!D.t3v.empty())
        std::memcpy(val3, D.t3v.data(), D.t3v.size() * 8);
    if (!D.d1v.empty())
        std::memcpy(val1, D.d1v.data(), D.d1v.size() * 8);
    sizes[0] = (int64_t)D.t3.size();
    sizes[1] = (int64_t)D.d1.size();
    sizes[2] = D.uncoded_reads;
    return 0;
}

// rf_host_upload_chunks: the chunk ends of one upload by either path
inline int host_upload_chunks(int32_t nseq, const int64_t *off, const int64_t *cins_off, const int64_t *cdel_off,
                              int32_t codes, int32_t stage_kb, int64_t budget, int32_t *end, int32_t *nchunks)
{
    if (nseq < 0 || !nchunks || (nseq > 0 && (!off || !end)) || (codes && (cins_off || cdel_off)))
        return RF_ERR_ARG;
    if (budget <= 0)
        budget = codes ? codes_stage_budget(stage_kb) : tables_stage_budget(stage_kb);
    *nchunks = 0;
    for (int32_t k0 = 0; k0 < nseq; k0 = end[*nchunks - 1])
        end[(*nchunks)++] = chunk_end(k0, nseq, budget, [&](int32_t k) {
            const int64_t n = off[k + 1] - off[k];
            return codes ? codes_stage_bytes(n)
                         : tables_stage_bytes(n, cins_off ? cins_off[k + 1] - cins_off[k] : 0,
                                              cdel_off ? cdel_off[k + 1] - cdel_off[k] : 0);
        });
    return 0;
}

#endif

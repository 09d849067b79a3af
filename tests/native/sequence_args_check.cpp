// Stand-alone check of the argument decisions of the sequence-model entry points (csrc/sequence_args.hpp: host only, no HIP): the
// list check at its limits and with two faults at once, the model-table and duration-table checks on NaN, -inf and values beyond
// the quantiser's clamp, in both diagonal modes, and the NULL and misaligned scans with optional pointers.  Built with
// -fsanitize=address,undefined by tests/test_sequence_entries.py: every array here is exactly as long as the function under
// test may read.  Any failed property or sanitizer report ends the run non-zero.
#include "sequence_args.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

using namespace hssfsst::seqargs;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { if (failures < 40) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } \
    } while (0)

static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kInf = std::numeric_limits<float>::infinity();

static constexpr int64_t mx = 1000;                      // the step limit of a recording in list_checks()

static bool is(const ListFinding& f, ListFault fault, int64_t index) { return f.fault == fault && (fault == ListFault::kNone || f.index == index); }

static void list_checks()
{
    const char* name = "list";
    auto run = [](std::vector<int64_t> offs, int64_t limit = mx) { return check_list(offs.data(), static_cast<int64_t>(offs.size()) - 1, limit); };
    CHECK(is(run({0}), ListFault::kNone, 0), "count 0");
    CHECK(is(run({3}), ListFault::kFirstNotZero, 0), "count 0, offsets[0] = 3");
    CHECK(is(run({0, 1}), ListFault::kNone, 0), "count 1");
    CHECK(is(run({0, 0}), ListFault::kNotIncreasing, 0), "count 1, empty");
    CHECK(is(run({0, -2}), ListFault::kNotIncreasing, 0), "count 1, reversed");
    CHECK(is(run({0, mx}), ListFault::kNone, 0), "the limit hit exactly");
    CHECK(is(run({0, mx + 1}), ListFault::kRecordingTooLong, 0), "the limit exceeded by one");
    CHECK(is(run({0, 5, 5 + mx, 6 + 2 * mx}), ListFault::kRecordingTooLong, 2), "the limit exceeded by one at recording 2");
    // the total: 2^31 - 1 passes, 2^31 does not
    const int64_t big = int64_t(1) << 26, n = (int64_t(1) << 31) / big;
    std::vector<int64_t> offs;
    for (int64_t i = 0; i <= n; ++i) offs.push_back(i * big);
    CHECK(is(run(offs, big), ListFault::kTooManySteps, n), "2^31 steps in all");
    offs.back() -= 1;
    CHECK(is(run(offs, big), ListFault::kNone, 0), "2^31 - 1 steps in all");
    CHECK(kMaxTotalSteps == (int64_t(1) << 31) - 1, "kMaxTotalSteps");
    // two faults at once: offsets[0], then a non-increase ANYWHERE, then the lowest recording over the limit, then the total
    CHECK(is(run({2, 1}), ListFault::kFirstNotZero, 0), "offsets[0] before a reversal");
    CHECK(is(run({1, mx + 9}), ListFault::kFirstNotZero, 0), "offsets[0] before the limit");
    CHECK(is(run({0, mx + 1, mx + 2, mx + 2}), ListFault::kNotIncreasing, 2), "a non-increase at 2 before the limit at 0");
    CHECK(is(run({0, 0, 4, 4}), ListFault::kNotIncreasing, 0), "the lowest non-increase");
    CHECK(is(run({0, mx + 1, mx + 2, 2 * mx + 9}), ListFault::kRecordingTooLong, 0), "the lowest recording over the limit");
    offs.back() += 2;                                    // the last recording one step over, 2^31 + 1 in all
    CHECK(is(run(offs, big), ListFault::kRecordingTooLong, n - 1), "the limit before the total");
    offs.push_back(offs.back());
    CHECK(is(run(offs, big + 1), ListFault::kNotIncreasing, n), "a non-increase before the total");
}

static void model_checks()
{
    const char* name = "model";
    std::vector<float> A(16, -kInf), pi(4, 0.0f);
    for (int i = 0; i < 4; ++i) A[4 * i + i] = A[4 * i + (i + 1) % 4] = 0.0f;               // the cardiac cycle: stay or advance
    for (int diag = 0; diag < 2; ++diag) {
        ModelFinding f = check_model(A.data(), pi.data(), diag != 0);
        CHECK(f.nan_at == -1 && f.dead_row == -1 && !f.no_start, "the cycle, diag %d: %d %d %d", diag, f.nan_at, f.dead_row, f.no_start);
        // NaN: the first one, transitions before initial, and found whatever else is wrong
        std::vector<float> a = A, p = pi;
        a[4 * 3 + 1] = kNaN;
        p[2] = kNaN;
        CHECK(check_model(a.data(), pi.data(), diag != 0).nan_at == 13, "NaN at [3][1]");
        CHECK(check_model(A.data(), p.data(), diag != 0).nan_at == 18, "NaN at initial[2]");
        CHECK(check_model(a.data(), p.data(), diag != 0).nan_at == 13, "transitions before initial");
        a[2] = kNaN;
        CHECK(check_model(a.data(), p.data(), diag != 0).nan_at == 2, "the first NaN");
        for (int j = 0; j < 4; ++j) a[4 + j] = -kInf;
        f = check_model(a.data(), p.data(), diag != 0);
        CHECK(f.nan_at == 2 && f.dead_row == 1, "a NaN and a dead row: both found (%d, %d)", f.nan_at, f.dead_row);
        // -inf is forbidden; values beyond the clamp, +inf and NaN are not (NaN counts as -32768, and is reported on its own)
        a = A;
        for (int j = 0; j < 4; ++j) a[8 + j] = -kInf;
        f = check_model(a.data(), pi.data(), diag != 0);
        CHECK(f.dead_row == 2 && f.nan_at == -1, "row 2 all -inf");
        for (int j = 0; j < 4; ++j) a[j] = -kInf;
        CHECK(check_model(a.data(), pi.data(), diag != 0).dead_row == 0, "the first dead row");
        for (float v : {-1e30f, -32769.0f, 1e30f, kInf, -std::numeric_limits<float>::max()}) {
            a = A;
            for (int j = 0; j < 4; ++j) a[8 + j] = v;
            p.assign(4, v);
            f = check_model(a.data(), p.data(), diag != 0);
            CHECK(f.dead_row == -1 && !f.no_start && f.nan_at == -1, "%g is not forbidden", static_cast<double>(v));
        }
        p.assign(4, -kInf);
        CHECK(check_model(A.data(), p.data(), diag != 0).no_start, "initial all -inf");
        p[3] = -40000.0f;
        CHECK(!check_model(A.data(), p.data(), diag != 0).no_start, "initial with one clamped entry");
        f = check_model(a.data(), std::vector<float>(4, -kInf).data(), diag != 0);
        CHECK(f.no_start && f.dead_row == -1, "no_start alone");
    }
    // a row whose only finite entry is the diagonal: a successor where the diagonal is read, none where it is not
    std::vector<float> a = A;
    a[4 * 1 + 2] = -kInf;
    CHECK(check_model(a.data(), pi.data(), false).dead_row == -1, "diagonal only, diagonal read");
    CHECK(check_model(a.data(), pi.data(), true).dead_row == 1, "diagonal only, diagonal not read");
    a[4 * 1 + 1] = -kInf;
    a[4 * 1 + 0] = -1e30f;                               // beyond the clamp, off the diagonal: a successor in both modes
    CHECK(check_model(a.data(), pi.data(), false).dead_row == -1 && check_model(a.data(), pi.data(), true).dead_row == -1, "clamped off-diagonal");
    CHECK(forbidden(-kInf) && !forbidden(kNaN) && !forbidden(-1e38f) && !forbidden(0.0f) && !forbidden(kInf), "forbidden()");
}

static bool is(const TableFinding& f, TableFault fault, int row, int column = 0)
{
    return f.fault == fault && (fault == TableFault::kNone || (f.row == row && (fault != TableFault::kNaN || f.column == column)));
}

static void table_checks()
{
    const char* name = "table";
    for (int D : {1, 2, 7, 2048}) {
        std::vector<float> t(static_cast<size_t>(4) * D, 0.0f);
        CHECK(is(check_duration_table(t.data(), D), TableFault::kNone, 0), "zeros, D %d", D);
        std::vector<float> u = t;
        u[static_cast<size_t>(3) * D + D - 1] = kNaN;
        CHECK(is(check_duration_table(u.data(), D), TableFault::kNaN, 3, D - 1), "NaN in the last entry, D %d", D);
        u[static_cast<size_t>(1) * D] = kNaN;
        CHECK(is(check_duration_table(u.data(), D), TableFault::kNaN, 1, 0), "the first NaN, D %d", D);
        for (int d = 0; d < D; ++d) u[static_cast<size_t>(2) * D + d] = -kInf;
        CHECK(is(check_duration_table(u.data(), D), TableFault::kNaN, 1, 0), "a NaN in row 1 before a dead row 2, D %d", D);
        u[static_cast<size_t>(1) * D] = 0.0f;
        CHECK(is(check_duration_table(u.data(), D), TableFault::kDeadRow, 2), "a dead row 2 before a NaN in row 3, D %d", D);
        u[static_cast<size_t>(2) * D + D - 1] = kNaN;
        CHECK(is(check_duration_table(u.data(), D), TableFault::kNaN, 2, D - 1), "a NaN at the end of an otherwise dead row, D %d", D);
        for (float v : {-1e30f, -32769.0f, kInf}) {
            u = t;
            for (int d = 0; d < D; ++d) u[static_cast<size_t>(0) * D + d] = -kInf;
            u[static_cast<size_t>(D) - 1] = v;
            CHECK(is(check_duration_table(u.data(), D), TableFault::kNone, 0), "one allowed duration of %g, D %d", static_cast<double>(v), D);
        }
        u.assign(u.size(), -kInf);
        CHECK(is(check_duration_table(u.data(), D), TableFault::kDeadRow, 0), "all -inf, D %d", D);
    }
}

static void pointer_checks()
{
    const char* name = "pointers";
    alignas(16) static char buf[64];
    const void *a16 = buf, *a8 = buf + 8, *a4 = buf + 4, *a2 = buf + 2, *none = nullptr;
    CHECK(first_null({{"a", a16}, {"b", a2}}) == nullptr, "no NULL");
    CHECK(first_null({}) == nullptr, "an empty list");
    const char* got = first_null({{"a", a16}, {"b", none}, {"c", none}});
    CHECK(got && got[0] == 'b', "the first NULL");
    got = first_null({{"a", none}, {"b", none}});
    CHECK(got && got[0] == 'a', "the first NULL of two");
    got = first_null({{"work", none}, {"counts", none}});                                 // the order is the list's, not the signature's
    CHECK(got && got[0] == 'w', "work before counts");
    CHECK(first_misaligned({{"a", a16, 16}, {"b", a8, 8}, {"c", a4, 4}, {"d", a2, 2}, {"e", buf + 1}}).name == nullptr, "all aligned");
    CHECK(first_misaligned({}).name == nullptr, "an empty list");
    CHECK(first_misaligned({{"a", none, 16}, {"b", none, 8}}).name == nullptr, "an optional NULL is aligned");
    NamedPointer p = first_misaligned({{"a", a16, 16}, {"b", none, 16}, {"c", a8, 16}, {"d", a4, 8}});
    CHECK(p.name && p.name[0] == 'c' && p.alignment == 16 && p.pointer == a8, "the first misaligned behind an optional NULL");
    p = first_misaligned({{"a", a16, 16}, {"b", a4, 4}, {"c", a4, 8}, {"d", a2, 16}});
    CHECK(p.name && p.name[0] == 'c' && p.alignment == 8, "order before alignment");
    p = first_misaligned({{"a", a2, 4}});
    CHECK(p.name && p.name[0] == 'a' && p.alignment == 4, "2 mod 4");
}

int main()
{
    list_checks();
    model_checks();
    table_checks();
    pointer_checks();
    if (failures) {
        std::printf("sequence args check FAILED: %d\n", failures);
        return 1;
    }
    std::printf("sequence args check ok\n");
    return 0;
}

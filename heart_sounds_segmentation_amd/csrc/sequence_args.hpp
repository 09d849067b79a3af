// sequence_args.hpp -- what the sequence-model entry points (hssfsst.h: hssfsst_decode_states .. hssfsst_posteriors_durations_counts)
// decide about their arguments before any device work, as plain functions that return what they found: the wording and the error
// code are the caller's (sequence.hip: seq_check_*).  No HIP type and no HIP call here, so all of it also compiles into a
// stand-alone program (tests/native/sequence_args_check.cpp).  "Forbidden" is decode_layout.hpp's: a value that quantises to kNeg.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "decode_layout.hpp"

namespace hssfsst::seqargs {

// ---- The list: count + 1 host offsets from 0, strictly increasing, no recording over max_steps, kMaxTotalSteps in all ----------
constexpr int64_t kMaxTotalSteps = 0x7fffffffLL;         // a step's index in the arenas is an int
enum class ListFault { kNone, kFirstNotZero, kNotIncreasing, kRecordingTooLong, kTooManySteps };
struct ListFinding {
    ListFault fault;
    int64_t index;                                       // the recording offsets[index] .. offsets[index + 1]; count for the total
};

// Precedence: offsets[0], then the lowest recording that does not increase ANYWHERE in the list, then the lowest one over
// max_steps, then the total.  count >= 0; offsets[0 .. count] are read.
inline ListFinding check_list(const int64_t* offsets, int64_t count, int64_t max_steps)
{
    if (offsets[0] != 0) return {ListFault::kFirstNotZero, 0};
    for (int64_t i = 0; i < count; ++i)
        if (offsets[i + 1] <= offsets[i]) return {ListFault::kNotIncreasing, i};
    for (int64_t i = 0; i < count; ++i)
        if (offsets[i + 1] - offsets[i] > max_steps) return {ListFault::kRecordingTooLong, i};
    return {offsets[count] > kMaxTotalSteps ? ListFault::kTooManySteps : ListFault::kNone, count};
}

// ---- The model's tables: transitions (4, 4) and initial (4) ---------------------------------------------------------------------
inline bool forbidden(float v) { return declayout::quantise(v) == declayout::kNeg; }

struct ModelFinding {
    int nan_at;                                          // the first NaN: 0 .. 15 in transitions (row-major), 16 .. 19 in initial; or -1
    int dead_row;                                        // the first row of transitions with no allowed successor, or -1
    bool no_start;                                       // every entry of initial is forbidden
};

// diagonal_not_read: the explicit-duration model never follows a run by a run of the same state, so a row's successor must be
// off the diagonal.
inline ModelFinding check_model(const float* transitions, const float* initial, bool diagonal_not_read)
{
    ModelFinding f{-1, -1, true};
    for (int i = 0; i < 20 && f.nan_at < 0; ++i) {
        const float v = i < 16 ? transitions[i] : initial[i - 16];
        if (v != v) f.nan_at = i;
    }
    for (int i = 0; i < 4; ++i) {
        bool any = false;
        for (int j = 0; j < 4; ++j) any = any || (!(diagonal_not_read && j == i) && !forbidden(transitions[4 * i + j]));
        if (!any && f.dead_row < 0) f.dead_row = i;
        f.no_start = f.no_start && forbidden(initial[i]);
    }
    return f;
}

// ---- One duration table (4, D): the score of a run of state j lasting d = 1 .. D steps at [j][d - 1] ---------------------------
enum class TableFault { kNone, kNaN, kDeadRow };         // kDeadRow: a row with no allowed duration
struct TableFinding {
    TableFault fault;
    int row, column;                                     // of the NaN; of a dead row only the row
};

// Rows are looked at in order and each one in full: a NaN is found before a dead row behind it and after a dead row before it.
inline TableFinding check_duration_table(const float* table, int D)
{
    for (int j = 0; j < 4; ++j) {
        bool any = false;
        for (int d = 0; d < D; ++d) {
            const float v = table[static_cast<size_t>(j) * D + d];
            if (v != v) return {TableFault::kNaN, j, d};
            any = any || !forbidden(v);
        }
        if (!any) return {TableFault::kDeadRow, j, 0};
    }
    return {TableFault::kNone, 0, 0};
}

// ---- Pointers, in the order of the caller's list ------------------------------------------------------------------------------
struct NamedPointer {
    const char* name;
    const void* pointer;
    unsigned alignment = 1;                              // in bytes
};

// the first NULL's name, or nullptr
inline const char* first_null(std::initializer_list<NamedPointer> required)
{
    for (const NamedPointer& p : required)
        if (!p.pointer) return p.name;
    return nullptr;
}

// the first pointer that is no multiple of its alignment, or one without a name.  NULL is a multiple of everything: an optional
// output that is not asked for is aligned.
inline NamedPointer first_misaligned(std::initializer_list<NamedPointer> pointers)
{
    for (const NamedPointer& p : pointers)
        if (reinterpret_cast<uintptr_t>(p.pointer) % p.alignment != 0) return p;
    return {nullptr, nullptr};
}

}  // namespace hssfsst::seqargs

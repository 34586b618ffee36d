// pc_letters.h -- what an ADAPTER letter stands for: a 5-bit set over the read's Dna5 codes 0..4 (A, C, G, T/U, everything
// else), and the one test "does this read base match this adapter letter".  Written once for device and host; every table
// builder (pc_api.cpp upload_panel, pc_prefilter_plan.h eq_words) and both plain-int32 routines (pc_slow.h, pc_paths.h) take
// the rule from here, and Python reads it through pc_letter_set (include/porechop_amd.h).  There is no second IUPAC table.
//
//   wildcards off   the set holds the letter's own Dna5 code: the reference's equality, N == N included ('N', '-', 'R' and
//                   every other non-base are all code 4 and equal one another).
//   wildcards on    A C G T, U = T;  R = AG  Y = CT  S = CG  W = AT  K = GT  M = AC;  B = CGT  D = AGT  H = ACT  V = ACG;
//                   N = ACGT; either case; any other byte is the EMPTY set.  Bit 4 is never set: a read base that is not
//                   A/C/G/T/U matches nothing, not even N, so a stretch masked with '-' is never a hit.
// Read bytes stay Dna5 in both modes (pcc::dna5_code).
#pragma once
#include <stdint.h>

#include "pc_walk.h"

namespace pcl {

constexpr unsigned A = 1, C = 2, G = 4, T = 8, UNKNOWN = 16;

PC_HD unsigned iupac_set(uint8_t byte)
{
    switch (byte | 0x20) {              // ASCII letters: lower case
        case 'a': return A;
        case 'c': return C;
        case 'g': return G;
        case 't': case 'u': return T;
        case 'r': return A | G;
        case 'y': return C | T;
        case 's': return C | G;
        case 'w': return A | T;
        case 'k': return G | T;
        case 'm': return A | C;
        case 'b': return C | G | T;
        case 'd': return A | G | T;
        case 'h': return A | C | T;
        case 'v': return A | C | G;
        case 'n': return A | C | G | T;
        default: return 0;
    }
}

// the set of an adapter byte
PC_HD unsigned letter_set(uint8_t byte, bool wildcards)
{
    const unsigned s = iupac_set(byte);
    if (wildcards) return s;
    return (s == A || s == C || s == G || s == T) ? s : UNKNOWN;     // {Dna5 code}
}

// read_code: 0..4
PC_HD bool matches(unsigned set, int read_code) { return (set >> read_code) & 1u; }

// the set of an adapter letter given as its Dna5 code: wildcards off
PC_HD unsigned code_set(int dna5_code) { return 1u << dna5_code; }

// does the mode change what this adapter byte matches?  (Every byte that is not A/C/G/T/U.)
PC_HD bool degenerate(uint8_t byte) { return letter_set(byte, true) != letter_set(byte, false); }

}  // namespace pcl

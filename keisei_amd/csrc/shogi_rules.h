// The shogi rules the device kernels share, owned by the env (csrc/shogi_env.hip): the layout of a game's state row, the
// piece bytes, the termination reasons and the attack test over the board in LDS.  The mate search (csrc/mate.hip) judges
// "gives check" with the env's own helpers; every file that reads a state row takes its offsets from here.
#pragma once
#include "common.h"

// a state row: board[81] hands[14] side in_check pad[3] | ply u32 @100 | key u64 @104 | reps u32 @112 | games u32 @116
constexpr int kStateBytes = 128;
constexpr int kSideByte = 95, kCheckByte = 96, kPlyByte = 100, kKeyByte = 104;         // (the board starts the row, the hands follow at 81)

enum { PAWN = 1, LANCE, KNIGHT, SILVER, GOLD, BISHOP, ROOK, KING };
constexpr int WHITE_BIT = 0x10, PROM_BIT = 0x20;
enum { R_PROGRESS = 0, R_CHECKMATE, R_REPETITION, R_PERPETUAL, R_IMPASSE, R_MAXMOVES };   // step_result.rs:9-16

// directions: N NE E SE S SW W NW (spatial_action_mapper.rs:31-40); "N" is toward row 0
// (row, column) steps as 2-bit fields of two immediates: the tables are on dependent-load chains of the ray walks
__device__ __forceinline__ int dir_dr(int d) { return ((0x1A90 >> (2 * d)) & 3) - 1; }      // -1 -1 0 1 1 1 0 -1
__device__ __forceinline__ int dir_dc(int d) { return ((0x01A9 >> (2 * d)) & 3) - 1; }      //  0  1 1 1 0 -1 -1 -1

// step (low byte) and slide (high byte) direction sets of every piece byte, in board directions (attack.rs:56-113)
__host__ __device__ constexpr unsigned dirs_of(int pc) {
    const unsigned N = 1, NE = 2, E = 4, SE = 8, S = 16, SW = 32, W = 64, NW = 128, gold = N | NE | NW | E | W | S;
    const int t = pc & 15;
    const bool pr = pc & PROM_BIT, wh = pc & WHITE_BIT;
    unsigned st = 0, sl = 0;
    if (pr) {
        if (t == PAWN || t == LANCE || t == KNIGHT || t == SILVER) st = gold;
        else if (t == BISHOP) { st = N | E | S | W; sl = NE | SE | SW | NW; }
        else if (t == ROOK) { st = NE | SE | SW | NW; sl = N | E | S | W; }
    } else {
        if (t == PAWN) st = N;
        else if (t == LANCE) sl = N;
        else if (t == SILVER) st = N | NE | NW | SE | SW;
        else if (t == GOLD) st = gold;
        else if (t == BISHOP) sl = NE | SE | SW | NW;
        else if (t == ROOK) sl = N | E | S | W;
        else if (t == KING) st = 255;
    }
    if (wh) { st = ((st << 4) | (st >> 4)) & 255; sl = ((sl << 4) | (sl >> 4)) & 255; }
    return st | (sl << 8);
}

// the board in LDS (explicit address space: these helpers are not always inlined) with up to two squares replaced
typedef const __attribute__((address_space(3))) uint8_t* lds_board;
typedef const __attribute__((address_space(3))) uint16_t* lds_dirs;      // dirs_of() of every piece byte, in LDS
struct View { lds_board b; lds_dirs dirs; int o1, p1, o2, p2; };
__device__ __forceinline__ int at(const View& v, int sq) { return sq == v.o1 ? v.p1 : sq == v.o2 ? v.p2 : v.b[sq]; }

// is `sq` attacked by a piece of colour `by`?  Looks outward from the square: the first piece met along each of the
// eight lines attacks it if it steps (distance 1) or slides back along that line; plus the two knight origins.
// One probe = one line (d < 8) or one knight origin (d = 8, 9), so that ten lanes can share a test.
__device__ __forceinline__ bool attacked_from(const View& v, int sq, int by, int d) {
    const int r = sq / 9, c = sq % 9;
    if (d < 8) {
        const int dr = dir_dr(d), dc = dir_dc(d);
        const unsigned need = 1u << ((d + 4) & 7);
        int rr = r + dr, cc = c + dc, k = 1;
        while ((unsigned)rr < 9u && (unsigned)cc < 9u) {
            const int p = at(v, rr * 9 + cc);
            if (p) {
                if (((p >> 4) & 1) != by) return false;
                const unsigned m = v.dirs[p & 63];
                return (k == 1 && (m & need)) || ((m >> 8) & need);
            }
            rr += dr; cc += dc; ++k;
        }
        return false;
    }
    const int kr = by ? r - 2 : r + 2, kc = c + (d == 8 ? -1 : 1);
    return (unsigned)kr < 9u && (unsigned)kc < 9u && at(v, kr * 9 + kc) == (KNIGHT | (by ? WHITE_BIT : 0));
}

// Border rows of the E-chain's last block row (k_chol_resident, the co-resident builds): which filters carry the eleven regressor columns
// B = [Z_P | E_top] of the innovation lift along as rows of the chain matrix -- after the n_e pivots of Sigma_e those rows hold (L_e^-1 B)^T and
// their 11 x 11 corner -B^T Sigma_e^-1 B = -G11 -- where in the last 64-block the rows sit, and how many role workgroups a filter's update
// then needs.  Host only, standard library only (no HIP, no other eqf_*.hpp; the layout constants are repeated here and static_assert-ed
// against the device headers where both are seen): tests/border_host_main.cpp runs it under the sanitizers without a GPU.
#pragma once

namespace eqf::border {

constexpr int kBlock = 64;   // block-column width of the chains (kSB)
constexpr int kStage = 16;   // columns of one stage of a diagonal block's factorisation (kQB)
constexpr int kRows = 11;    // border rows: the six columns of Z_P, then the five of E_top
constexpr int kMaxStage = 3; // the border needs one whole unpivoted 16-row stage: at most three stages of the last block hold a real column

inline int eOrder(int N) { return 6 + 3 * N; }                       // order of Sigma_e in the padded index map (eDim)
inline int sOrder(int N) { return 2 * N; }                           // order of S (sDim)
inline int rhsColumns(int N) { return 12 + 3 * N + 6; }              // columns of the S-chain's right-hand side (yCols)
inline int blocks(int n) { return (n + kBlock - 1) / kBlock; }       // 64-wide block columns of a chain of order n
// stages of the chain's LAST diagonal block that hold a real column (realStages(eDim(N), 64 (nb - 1)))
inline int lastStages(int N) {
    const int rem = eOrder(N) - kBlock * (blocks(eOrder(N)) - 1);
    const int st = (rem + kStage - 1) / kStage;
    return st < 1 ? 1 : (st > 4 ? 4 : st);
}
// The stage of the last block whose first eleven rows are the border: the first one behind the real columns; -1 when fewer than sixteen
// unpivoted rows are left (the order of Sigma_e a multiple of 64, or more than 48 real rows in the last block).
inline int borderStage(int N) {
    const int nst = lastStages(N);
    return nst <= kMaxStage ? nst : -1;
}
// A filter takes the border when it has room for it and a row head to finish it (two block columns: N >= 20)
inline bool borderOn(int N) { return N > 0 && borderStage(N) >= 0 && blocks(eOrder(N)) >= 2; }
// row of the chain matrix that carries regressor column q
inline int borderRow(int N, int q) { return kBlock * (blocks(eOrder(N)) - 1) + kStage * borderStage(N) + q; }

// Role workgroups of one chain of nb block columns with wt right-hand-side column tiles: row heads, interior tiles, right-hand-side tiles
inline int chainRoles(int nb, int wt) { return (nb - 1) + (nb - 1) * (nb - 2) / 2 + wt * nb; }
// ... of a filter's update without the border (both chains; the first diagonal blocks and the prep roles are counted by the caller)
inline int rolesPlain(int N) { return chainRoles(blocks(sOrder(N)), blocks(rhsColumns(N))) + chainRoles(blocks(eOrder(N)), 1); }
// ... and with it: of the E-chain's right-hand-side tiles only the last one stays, as the workgroup that runs the lift
inline int rolesBorder(int N) { return borderOn(N) ? rolesPlain(N) - (blocks(eOrder(N)) - 1) : rolesPlain(N); }

// Which right-hand-side roles W(0, C) of the E-chain the role table of a batch may leave out: bit C is set when NO filter of the batch needs
// that role.  A filter without the border needs all of them up to its last block row, one with it only the last (the lift).  counts[b] <= 0:
// the filter takes no part.  More than 62 block columns: nothing is left out.
inline unsigned long long omitMask(const int* counts, int B, int nbMax) {
    if (nbMax < 2 || nbMax > 62) return 0ull;
    unsigned long long need = 0ull;
    for (int b = 0; b < B; ++b) {
        if (counts[b] <= 0) continue;
        const int nb = blocks(eOrder(counts[b]));
        if (nb > nbMax) return 0ull;
        if (borderOn(counts[b])) need |= 1ull << (nb - 1);
        else need |= (1ull << nb) - 1ull;
    }
    return ~need & ((1ull << nbMax) - 1ull);
}

}  // namespace eqf::border

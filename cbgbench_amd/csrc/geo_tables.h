// libcbgx -- what the translation units of the geometry reports share (geometry.hip, distributions.hip, interactions.hip, groups.hip): the limits, the element codes,
// the constant tables as a compile-time initialiser, and the fp64 squared distance.  The sources and the meaning of the constants are in
// the head of geometry.hip.  A translation unit that includes this keeps contraction off (#pragma clang fp contract(off)): geo_dist2's
// products and sums are plain operators.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"

namespace cbgx {

constexpr int GEO_THREADS = 256;
constexpr int GEO_MAX = CBGX_GEOMETRY_MAX_LIGAND;
constexpr int GEO_EL = 8;         // element codes 0..7 = H C N O F P S Cl: bond table, valences, radii
constexpr int GEO_VDW = 9;        // code 8 = Br: a radius only
constexpr int GEO_NONE = 255;     // no code
constexpr double GEO_FAR2 = 25.0; // squared distance from which no threshold can be met (see `shortcut` in geometry.hip)

enum : int { EL_H = 0, EL_C, EL_N, EL_O, EL_F, EL_P, EL_S, EL_CL, EL_BR };

struct GeoPair { int a, b, pm; };

struct GeoTables {
    int32_t bond_pm[3][GEO_EL][GEO_EL];   // [order - 1][code][code], -1: no such bond
    int32_t margin[3];
    int32_t allowed[GEO_EL];
    uint8_t z[GEO_VDW];                   // atomic number of a code
    double radius[GEO_VDW];
    double tolerance;
};

constexpr GeoTables make_geo_tables() {
    constexpr GeoPair single_pm[] = {
        {EL_H, EL_H, 74},   {EL_H, EL_C, 109},  {EL_H, EL_N, 101},  {EL_H, EL_O, 96},   {EL_H, EL_F, 92},   {EL_H, EL_P, 144},
        {EL_H, EL_S, 134},  {EL_H, EL_CL, 127}, {EL_C, EL_C, 154},  {EL_C, EL_N, 147},  {EL_C, EL_O, 143},  {EL_C, EL_F, 135},
        {EL_C, EL_P, 184},  {EL_C, EL_S, 182},  {EL_C, EL_CL, 177}, {EL_N, EL_N, 145},  {EL_N, EL_O, 140},  {EL_N, EL_F, 136},
        {EL_N, EL_P, 177},  {EL_N, EL_S, 168},  {EL_N, EL_CL, 175}, {EL_O, EL_O, 148},  {EL_O, EL_F, 142},  {EL_O, EL_P, 163},
        {EL_O, EL_S, 151},  {EL_O, EL_CL, 164}, {EL_F, EL_F, 142},  {EL_F, EL_P, 156},  {EL_F, EL_S, 158},  {EL_F, EL_CL, 166},
        {EL_P, EL_P, 221},  {EL_P, EL_S, 210},  {EL_P, EL_CL, 203}, {EL_S, EL_S, 204},  {EL_S, EL_CL, 207}, {EL_CL, EL_CL, 199}};
    constexpr GeoPair double_pm[] = {{EL_C, EL_C, 134}, {EL_C, EL_N, 129}, {EL_C, EL_O, 120}, {EL_C, EL_S, 160}, {EL_N, EL_N, 125},
                                     {EL_N, EL_O, 121}, {EL_O, EL_O, 121}, {EL_O, EL_P, 150}, {EL_P, EL_S, 186}};
    constexpr GeoPair triple_pm[] = {{EL_C, EL_C, 120}, {EL_C, EL_N, 116}, {EL_C, EL_O, 113}, {EL_N, EL_N, 110}};
    GeoTables t{};
    for (int o = 0; o < 3; ++o)
        for (int a = 0; a < GEO_EL; ++a)
            for (int b = 0; b < GEO_EL; ++b) t.bond_pm[o][a][b] = -1;
    for (const GeoPair& p : single_pm) t.bond_pm[0][p.a][p.b] = t.bond_pm[0][p.b][p.a] = p.pm;
    for (const GeoPair& p : double_pm) t.bond_pm[1][p.a][p.b] = t.bond_pm[1][p.b][p.a] = p.pm;
    for (const GeoPair& p : triple_pm) t.bond_pm[2][p.a][p.b] = t.bond_pm[2][p.b][p.a] = p.pm;
    t.margin[0] = 10; t.margin[1] = 5; t.margin[2] = 3;
    //                      H  C  N  O  F  P   S   Cl  Br
    constexpr int zs[] =   {1, 6, 7, 8, 9, 15, 16, 17, 35};
    constexpr int val[] =  {1, 4, 3, 2, 1, 5,  4,  1};
    constexpr double r[] = {1.2, 1.7, 1.55, 1.52, 1.47, 1.8, 1.8, 2.27, 1.85};
    for (int c = 0; c < GEO_VDW; ++c) { t.z[c] = (uint8_t)zs[c]; t.radius[c] = r[c]; }
    for (int c = 0; c < GEO_EL; ++c) t.allowed[c] = val[c];
    t.tolerance = 0.4;
    return t;
}

// ---- the interaction report (interactions.hip; the definition is in include/cbgx.h, cbgx_pocket_types / cbgx_ligand_interactions) ------
// A type byte: the element code 1 ... 7 (C N O F P S Cl; 0: takes no part) in its low three bits, and the three property bits.
constexpr int IA_RES = 20;        // residue indices 0 ... 19 in the reference's aa_name_number order; index IA_RES stands for any other

enum : int { AA_ALA = 0, AA_CYS, AA_ASP, AA_GLU, AA_PHE, AA_GLY, AA_HIS, AA_ILE, AA_LYS, AA_LEU, AA_MET, AA_ASN, AA_PRO, AA_GLN, AA_ARG,
             AA_SER, AA_THR, AA_VAL, AA_TRP, AA_TYR };

struct InteractionTables {
    double radius[GEO_EL];                // Vina's atom radii by element code (Trott & Olson 2010); 0 for H
    double c_bond[4];                     // [1 N, 2 O, 3 S]: the C-X single bond length + margin in pm, as the fp64 value p is compared with
    uint8_t n_type[2][IA_RES + 1];        // [backbone][residue] property bits of a pocket nitrogen
    uint8_t o_type[2][IA_RES + 1];        // ... of a pocket oxygen
};

constexpr InteractionTables make_interaction_tables() {
    constexpr uint8_t don = CBGX_INTERACTIONS_DONOR, acc = CBGX_INTERACTIONS_ACCEPTOR;
    constexpr int n_donor_side[] = {AA_LYS, AA_ARG, AA_ASN, AA_GLN, AA_TRP};
    constexpr int o_donor_side[] = {AA_SER, AA_THR, AA_TYR};
    InteractionTables t{};
    //                        H    C    N    O    F    P    S    Cl
    constexpr double r[] = {0.0, 1.9, 1.8, 1.7, 1.5, 2.1, 2.0, 1.8};
    for (int c = 0; c < GEO_EL; ++c) t.radius[c] = r[c];
    const GeoTables geo = make_geo_tables();
    t.c_bond[0] = 0.0;
    t.c_bond[1] = (double)(geo.bond_pm[0][EL_C][EL_N] + geo.margin[0]);
    t.c_bond[2] = (double)(geo.bond_pm[0][EL_C][EL_O] + geo.margin[0]);
    t.c_bond[3] = (double)(geo.bond_pm[0][EL_C][EL_S] + geo.margin[0]);
    for (int a = 0; a <= IA_RES; ++a) {
        t.n_type[0][a] = 0;               // side chain: neither, but for the residues below
        t.n_type[1][a] = don;             // backbone N-H
        t.o_type[0][a] = t.o_type[1][a] = acc;
    }
    t.n_type[1][AA_PRO] = 0;              // no hydrogen on proline's ring nitrogen
    for (int a : n_donor_side) t.n_type[0][a] = don;
    t.n_type[0][AA_HIS] = don | acc;      // no protonation state: both, always
    for (int a : o_donor_side) t.o_type[0][a] = don | acc;
    return t;
}

// ---- the functional-group report (groups.hip; the definition is in include/cbgx.h, cbgx_ligand_groups) ----------------------------------
// A template is a labelled graph: an atom label is (element code << 1) | aromatic bit, a bond is (atom, atom, type 1 ... 4).  The atoms of
// every template are listed so that each one after the first has a bond to an earlier one: the matcher extends a connected partial map.
constexpr int GRP_CLASSES = CBGX_GROUPS_CLASSES;        // named classes; index GRP_CLASSES is `other`
constexpr int GRP_T_ATOMS = CBGX_GROUPS_MAX_TEMPLATE_ATOMS;
constexpr int GRP_T_BONDS = CBGX_GROUPS_MAX_TEMPLATE_BONDS;   // naphthalene, quinoline

enum : uint8_t { GL_C = EL_C << 1, GL_c = (EL_C << 1) | 1, GL_N = EL_N << 1, GL_n = (EL_N << 1) | 1, GL_O = EL_O << 1, GL_P = EL_P << 1,
                 GL_S = EL_S << 1, GL_s = (EL_S << 1) | 1 };

struct GroupBond { uint8_t i, j, t; };

struct GroupTemplate {
    uint8_t n_atoms, n_bonds;
    uint8_t label[GRP_T_ATOMS];
    GroupBond bond[GRP_T_BONDS];
};

struct GroupTables {
    GroupTemplate t[GRP_CLASSES];
    uint64_t hist[GRP_CLASSES];                       // 4 bits per label: how many atoms carry it (the sorted labels, as one number)
    uint8_t adj[GRP_CLASSES][GRP_T_ATOMS][GRP_T_ATOMS]; // bond type between two template atoms, 0: none
};

constexpr GroupTables make_group_tables() {
    // a ring of n atoms 0 ... n - 1 is the bonds (k, k + 1) and (0, n - 1), type 4; fused systems add their closing bonds
    constexpr GroupTemplate list[GRP_CLASSES] = {
        /*  0 c1ccccc1             */ {6, 6, {GL_c, GL_c, GL_c, GL_c, GL_c, GL_c}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {0, 5, 4}}},
        /*  1 NC=O                 */ {3, 2, {GL_N, GL_C, GL_O}, {{0, 1, 1}, {1, 2, 2}}},
        /*  2 O=CO                 */ {3, 2, {GL_O, GL_C, GL_O}, {{0, 1, 2}, {1, 2, 1}}},
        /*  3 c1ccncc1             */ {6, 6, {GL_c, GL_c, GL_c, GL_n, GL_c, GL_c}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {0, 5, 4}}},
        /*  4 c1ncc2nc[nH]c2n1     */ {9, 10, {GL_c, GL_n, GL_c, GL_c, GL_n, GL_c, GL_n, GL_c, GL_n},
                                       {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {5, 6, 4}, {6, 7, 4}, {3, 7, 4}, {7, 8, 4}, {0, 8, 4}}},
        /*  5 NS(=O)=O             */ {4, 3, {GL_N, GL_S, GL_O, GL_O}, {{0, 1, 1}, {1, 2, 2}, {1, 3, 2}}},
        /*  6 O=P(O)(O)O           */ {5, 4, {GL_O, GL_P, GL_O, GL_O, GL_O}, {{0, 1, 2}, {1, 2, 1}, {1, 3, 1}, {1, 4, 1}}},
        /*  7 OCO                  */ {3, 2, {GL_O, GL_C, GL_O}, {{0, 1, 1}, {1, 2, 1}}},
        /*  8 c1cncnc1             */ {6, 6, {GL_c, GL_c, GL_n, GL_c, GL_n, GL_c}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {0, 5, 4}}},
        /*  9 c1cn[nH]c1           */ {5, 5, {GL_c, GL_c, GL_n, GL_n, GL_c}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {0, 4, 4}}},
        /* 10 O=P(O)O              */ {4, 3, {GL_O, GL_P, GL_O, GL_O}, {{0, 1, 2}, {1, 2, 1}, {1, 3, 1}}},
        /* 11 c1ccc2ccccc2c1       */ {10, 11, {GL_c, GL_c, GL_c, GL_c, GL_c, GL_c, GL_c, GL_c, GL_c, GL_c},
                                       {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {5, 6, 4}, {6, 7, 4}, {7, 8, 4}, {3, 8, 4}, {8, 9, 4}, {0, 9, 4}}},
        /* 12 c1ccsc1              */ {5, 5, {GL_c, GL_c, GL_c, GL_s, GL_c}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {0, 4, 4}}},
        /* 13 N=CN                 */ {3, 2, {GL_N, GL_C, GL_N}, {{0, 1, 2}, {1, 2, 1}}},
        /* 14 NC(N)=O              */ {4, 3, {GL_N, GL_C, GL_N, GL_O}, {{0, 1, 1}, {1, 2, 1}, {1, 3, 2}}},
        /* 15 O=c1cc[nH]c(=O)[nH]1 */ {8, 8, {GL_O, GL_c, GL_c, GL_c, GL_n, GL_c, GL_O, GL_n},
                                       {{0, 1, 2}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {5, 6, 2}, {5, 7, 4}, {1, 7, 4}}},
        /* 16 c1ccc2ncccc2c1       */ {10, 11, {GL_c, GL_c, GL_c, GL_c, GL_n, GL_c, GL_c, GL_c, GL_c, GL_c},
                                       {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {5, 6, 4}, {6, 7, 4}, {7, 8, 4}, {3, 8, 4}, {8, 9, 4}, {0, 9, 4}}},
        /* 17 c1cscn1              */ {5, 5, {GL_c, GL_c, GL_s, GL_c, GL_n}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {0, 4, 4}}},
        /* 18 c1ccc2[nH]cnc2c1     */ {9, 10, {GL_c, GL_c, GL_c, GL_c, GL_n, GL_c, GL_n, GL_c, GL_c},
                                       {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {5, 6, 4}, {6, 7, 4}, {3, 7, 4}, {7, 8, 4}, {0, 8, 4}}},
        /* 19 c1c[nH]cn1           */ {5, 5, {GL_c, GL_c, GL_n, GL_c, GL_n}, {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {0, 4, 4}}},
        /* 20 O=[N+][O-]           */ {3, 2, {GL_O, GL_N, GL_O}, {{0, 1, 2}, {1, 2, 2}}},       // no charges here: the graph N(=O)=O
        /* 21 O=CNO                */ {4, 3, {GL_O, GL_C, GL_N, GL_O}, {{0, 1, 2}, {1, 2, 1}, {2, 3, 1}}},
        /* 22 NC(=O)O              */ {4, 3, {GL_N, GL_C, GL_O, GL_O}, {{0, 1, 1}, {1, 2, 2}, {1, 3, 1}}},
        /* 23 O=S=O                */ {3, 2, {GL_O, GL_S, GL_O}, {{0, 1, 2}, {1, 2, 2}}},
        /* 24 c1ccc2[nH]ccc2c1     */ {9, 10, {GL_c, GL_c, GL_c, GL_c, GL_n, GL_c, GL_c, GL_c, GL_c},
                                       {{0, 1, 4}, {1, 2, 4}, {2, 3, 4}, {3, 4, 4}, {4, 5, 4}, {5, 6, 4}, {6, 7, 4}, {3, 7, 4}, {7, 8, 4}, {0, 8, 4}}}};
    GroupTables g{};
    for (int k = 0; k < GRP_CLASSES; ++k) {
        g.t[k] = list[k];
        for (int a = 0; a < list[k].n_atoms; ++a) g.hist[k] += 1ull << (4 * list[k].label[a]);
        for (int b = 0; b < list[k].n_bonds; ++b) {
            const GroupBond e = list[k].bond[b];
            g.adj[k][e.i][e.j] = g.adj[k][e.j][e.i] = e.t;
        }
    }
    return g;
}

// squared distance in fp64 from fp32 coordinates, each operation rounded on its own
__device__ __forceinline__ double geo_dist2(double ax, double ay, double az, float bx, float by, float bz) {
    const double dx = ax - (double)bx, dy = ay - (double)by, dz = az - (double)bz;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}

}  // namespace cbgx

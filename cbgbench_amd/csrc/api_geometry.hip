// libcbgx -- C ABI of the geometry report, of the bond list, of the ring sizes, of the aromatic report, of the valence report, of the
// interaction report, of the functional groups, of the fingerprints, of the comparison with a native ligand and of the distributions
// (include/cbgx.h, geometry.hip, rings.hip, aromatic.hip, valence.hip, interactions.hip, groups.hip, diversity.hip, native.hip,
// distributions.hip): argument checks, the ligand-size check, the launch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/cbgx.h"
#include "kernels.h"

namespace cbgx { int set_error(int code, const char* fmt, ...); }
using namespace cbgx;

// lig_ptr [count] on the host.  Device (or managed) memory: a copy on the caller's stream and a wait for it.  Pinned host memory: read in
// place.  Anything the runtime does not know -- plain host memory, or no device at all -- is read in place too and reported as not
// visible to the device, so that the size check works without one and nothing is launched on such a pointer.
static int fetch_csr(const char* who, const int32_t* p, int count, std::vector<int32_t>& host, bool& device_visible, hipStream_t s) {
    host.resize((size_t)count);
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e == hipSuccess && attr.type != hipMemoryTypeUnregistered && attr.type != hipMemoryTypeHost) {
        device_visible = true;
        hipError_t c = hipMemcpyAsync(host.data(), p, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, s);
        if (c == hipSuccess) c = hipStreamSynchronize(s);
        if (c != hipSuccess) return set_error(CBGX_E_HIP, "%s: reading lig_ptr: %s", who, hipGetErrorString(c));
        return CBGX_OK;
    }
    device_visible = e == hipSuccess && attr.type == hipMemoryTypeHost;
    if (e != hipSuccess) (void)hipGetLastError();      // not an error of this call: the pointer is simply not the runtime's
    memcpy(host.data(), p, sizeof(int32_t) * (size_t)count);
    return CBGX_OK;
}

// what every entry does between its argument checks and its launch: the read-back of lig_ptr, the size check over the ranges the kernels
// use (clamped to the array), and the refusal of a lig_ptr no kernel could read
static int check_ligand_sizes(const char* who, const int32_t* lig_ptr, int n_lig, int n_graphs, hipStream_t s) {
    std::vector<int32_t> ptr;
    bool device_visible = false;
    const int rc = fetch_csr(who, lig_ptr, n_graphs + 1, ptr, device_visible, s);
    if (rc != CBGX_OK) return rc;
    for (int g = 0; g < n_graphs; ++g) {
        const int l0 = std::min(std::max(ptr[g], 0), n_lig), l1 = std::min(std::max(ptr[g + 1], l0), n_lig);
        if (l1 - l0 > CBGX_GEOMETRY_MAX_LIGAND)
            return set_error(CBGX_E_INVALID, "%s: graph %d has %d ligand atoms, more than the %d one workgroup stages", who, g, l1 - l0,
                             CBGX_GEOMETRY_MAX_LIGAND);
    }
    if (!device_visible) return set_error(CBGX_E_INVALID, "%s: lig_ptr is not memory the device can read", who);
    return CBGX_OK;
}

extern "C" {

int cbgx_ligand_geometry(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                         const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, int32_t* nr_bonds, uint8_t* flags,
                         int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_rec < 0)
        return set_error(CBGX_E_INVALID, "ligand_geometry: negative count (B=%d n_lig=%d n_rec=%d)", n_graphs, n_lig, n_rec);
    if ((n_graphs > 0 && (!lig_ptr || !rec_ptr || !graph_out)) || (n_lig > 0 && (!x_lig || !z_lig || !nr_bonds || !flags)) ||
        (n_rec > 0 && (!x_rec || !z_rec)))
        return set_error(CBGX_E_INVALID, "ligand_geometry: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const int rc = check_ligand_sizes("ligand_geometry", lig_ptr, n_lig, n_graphs, (hipStream_t)stream);
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_geometry(x_lig, z_lig, lig_ptr, n_lig, x_rec, z_rec, rec_ptr, n_rec, n_graphs, nr_bonds, flags,
                                                graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_geometry: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_bonds_count(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, int32_t* deg_up,
                            int32_t* fragment, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0) return set_error(CBGX_E_INVALID, "ligand_bonds_count: negative count (B=%d n_lig=%d)", n_graphs, n_lig);
    if ((n_graphs > 0 && (!lig_ptr || !graph_out)) || (n_lig > 0 && (!x_lig || !z_lig || !deg_up || !fragment)))
        return set_error(CBGX_E_INVALID, "ligand_bonds_count: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const int rc = check_ligand_sizes("ligand_bonds_count", lig_ptr, n_lig, n_graphs, (hipStream_t)stream);
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_bonds_count(x_lig, z_lig, lig_ptr, n_lig, n_graphs, deg_up, fragment, graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_bonds_count: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_bonds_fill(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                           const int32_t* bond_ptr, int n_bonds, int32_t* bond_index, uint8_t* bond_order, double* bond_length,
                           void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_bonds_fill: negative count (B=%d n_lig=%d n_bonds=%d)", n_graphs, n_lig, n_bonds);
    if ((n_graphs > 0 && (!lig_ptr || !bond_ptr)) || (n_lig > 0 && (!x_lig || !z_lig)) ||
        (n_bonds > 0 && (!bond_index || !bond_order || !bond_length)))
        return set_error(CBGX_E_INVALID, "ligand_bonds_fill: NULL pointer");
    if (n_graphs == 0 || n_bonds == 0) return CBGX_OK;
    const int rc = check_ligand_sizes("ligand_bonds_fill", lig_ptr, n_lig, n_graphs, (hipStream_t)stream);
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_bonds_fill(x_lig, z_lig, lig_ptr, n_lig, n_graphs, bond_ptr, n_bonds, bond_index, bond_order,
                                                  bond_length, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_bonds_fill: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_rings(const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr, const int32_t* bond_index, int n_bonds,
                      uint8_t* atom_ring_min, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_rings: negative count (B=%d n_lig=%d n_bonds=%d)", n_graphs, n_lig, n_bonds);
    if ((n_graphs > 0 && (!lig_ptr || !bond_ptr || !graph_out)) || (n_lig > 0 && !atom_ring_min) || (n_bonds > 0 && !bond_index))
        return set_error(CBGX_E_INVALID, "ligand_rings: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    // no size is refused here (a graph over a limit is reported in its status), so lig_ptr is not read back: only whether the kernel could
    hipPointerAttribute_t attr;
    const hipError_t known = hipPointerGetAttributes(&attr, lig_ptr);
    if (known != hipSuccess) (void)hipGetLastError();      // not an error of this call: the pointer is simply not the runtime's
    if (known != hipSuccess || attr.type == hipMemoryTypeUnregistered)
        return set_error(CBGX_E_INVALID, "ligand_rings: lig_ptr is not memory the device can read");
    const hipError_t e = launch_ligand_rings(lig_ptr, n_lig, n_graphs, bond_ptr, bond_index, n_bonds, atom_ring_min, graph_out,
                                             (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_rings: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_aromatic(const uint8_t* z_lig, const uint8_t* flag_lig, const uint8_t* atom_ring_min, const int32_t* lig_ptr, int n_lig,
                         int n_graphs, const int32_t* bond_ptr, const int32_t* bond_index, int n_bonds, uint8_t* atom_out,
                         uint8_t* bond_aromatic, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_aromatic: negative count (B=%d n_lig=%d n_bonds=%d)", n_graphs, n_lig, n_bonds);
    if ((n_graphs > 0 && (!lig_ptr || !bond_ptr || !graph_out)) || (n_lig > 0 && (!z_lig || !flag_lig || !atom_ring_min || !atom_out)) ||
        (n_bonds > 0 && (!bond_index || !bond_aromatic)))
        return set_error(CBGX_E_INVALID, "ligand_aromatic: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    // no size is refused here (a graph over a limit is reported in its status), so lig_ptr is not read back: only whether the kernel could
    hipPointerAttribute_t attr;
    const hipError_t known = hipPointerGetAttributes(&attr, lig_ptr);
    if (known != hipSuccess) (void)hipGetLastError();      // not an error of this call: the pointer is simply not the runtime's
    if (known != hipSuccess || attr.type == hipMemoryTypeUnregistered)
        return set_error(CBGX_E_INVALID, "ligand_aromatic: lig_ptr is not memory the device can read");
    const hipError_t e = launch_ligand_aromatic(z_lig, flag_lig, atom_ring_min, lig_ptr, n_lig, n_graphs, bond_ptr, bond_index, n_bonds,
                                                atom_out, bond_aromatic, graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_aromatic: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_valence(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                        const int32_t* bond_index, const uint8_t* bond_order, const uint8_t* bond_aromatic, int n_bonds, int max_steps,
                        uint8_t* implicit_h, uint8_t* atom_flags, uint8_t* bond_kekule, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_valence: negative count (B=%d n_lig=%d n_bonds=%d)", n_graphs, n_lig, n_bonds);
    if (max_steps < 1 || max_steps > CBGX_VALENCE_MAX_STEPS)
        return set_error(CBGX_E_INVALID, "ligand_valence: max_steps=%d outside 1 ... %d", max_steps, CBGX_VALENCE_MAX_STEPS);
    if ((n_graphs > 0 && (!lig_ptr || !bond_ptr || !graph_out)) || (n_lig > 0 && (!z_lig || !implicit_h || !atom_flags)) ||
        (n_bonds > 0 && (!bond_index || !bond_order || !bond_kekule)))
        return set_error(CBGX_E_INVALID, "ligand_valence: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    // no size is refused here (a graph over a limit is reported in its status), so lig_ptr is not read back: only whether the kernel could
    hipPointerAttribute_t attr;
    const hipError_t known = hipPointerGetAttributes(&attr, lig_ptr);
    if (known != hipSuccess) (void)hipGetLastError();      // not an error of this call: the pointer is simply not the runtime's
    if (known != hipSuccess || attr.type == hipMemoryTypeUnregistered)
        return set_error(CBGX_E_INVALID, "ligand_valence: lig_ptr is not memory the device can read");
    const hipError_t e = launch_ligand_valence(z_lig, lig_ptr, n_lig, n_graphs, bond_ptr, bond_index, bond_order, bond_aromatic, n_bonds,
                                               max_steps, implicit_h, atom_flags, bond_kekule, graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_valence: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

// no size is refused by the two interaction entries (a graph over a limit is reported in its status), so no CSR is read back: only
// whether the kernel could touch what it is handed.  EVERY array with a non-zero count is asked for, in argument order: a pointer the
// runtime does not know (plain host memory) is refused here and never reaches a launch
struct DeviceArray { const char* name; const void* p; int count; };

static int device_visible(const char* who, const DeviceArray* arrays, int n_arrays) {
    for (int a = 0; a < n_arrays; ++a) {
        if (!arrays[a].p || arrays[a].count <= 0) continue;
        hipPointerAttribute_t attr;
        const hipError_t known = hipPointerGetAttributes(&attr, arrays[a].p);
        if (known != hipSuccess) (void)hipGetLastError();      // not an error of this call: the pointer is simply not the runtime's
        if (known != hipSuccess || attr.type == hipMemoryTypeUnregistered)
            return set_error(CBGX_E_INVALID, "%s: %s is not memory the device can read", who, arrays[a].name);
    }
    return CBGX_OK;
}

int cbgx_pocket_types(const float* x_rec, const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, const uint8_t* rec_aa,
                      const uint8_t* rec_backbone, uint8_t* rec_type, void* stream) {
    if (n_graphs < 0 || n_rec < 0) return set_error(CBGX_E_INVALID, "pocket_types: negative count (B=%d n_rec=%d)", n_graphs, n_rec);
    if ((n_graphs > 0 && !rec_ptr) || (n_rec > 0 && (!x_rec || !z_rec || !rec_aa || !rec_backbone || !rec_type)))
        return set_error(CBGX_E_INVALID, "pocket_types: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const DeviceArray arrays[] = {{"rec_ptr", rec_ptr, n_graphs + 1}, {"x_rec", x_rec, n_rec}, {"z_rec", z_rec, n_rec},
                                  {"rec_aa", rec_aa, n_rec}, {"rec_backbone", rec_backbone, n_rec}, {"rec_type", rec_type, n_rec}};
    const int rc = device_visible("pocket_types", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_pocket_types(x_rec, z_rec, rec_ptr, n_rec, n_graphs, rec_aa, rec_backbone, rec_type, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "pocket_types: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_interactions(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                             const uint8_t* rec_type, const int32_t* rec_ptr, int n_rec, int n_graphs, const int32_t* bond_ptr,
                             const int32_t* bond_index, const uint8_t* bond_kekule, const uint8_t* bond_aromatic, int n_bonds,
                             const uint8_t* implicit_h, const uint8_t* atom_flags, const int32_t* valence_status, double* atom_terms,
                             uint8_t* lig_type, uint8_t* bond_rotatable, double* graph_terms, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_rec < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_interactions: negative count (B=%d n_lig=%d n_rec=%d n_bonds=%d)", n_graphs, n_lig, n_rec,
                         n_bonds);
    if ((n_graphs > 0 && (!lig_ptr || !rec_ptr || !bond_ptr || !valence_status || !graph_terms || !graph_out)) ||
        (n_lig > 0 && (!x_lig || !z_lig || !implicit_h || !atom_flags || !atom_terms || !lig_type)) || (n_rec > 0 && (!x_rec || !rec_type)) ||
        (n_bonds > 0 && (!bond_index || !bond_kekule || !bond_rotatable)))
        return set_error(CBGX_E_INVALID, "ligand_interactions: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const DeviceArray arrays[] = {
        {"lig_ptr", lig_ptr, n_graphs + 1}, {"x_lig", x_lig, n_lig}, {"z_lig", z_lig, n_lig}, {"x_rec", x_rec, n_rec},
        {"rec_type", rec_type, n_rec}, {"rec_ptr", rec_ptr, n_graphs + 1}, {"bond_ptr", bond_ptr, n_lig + 1},
        {"bond_index", bond_index, n_bonds}, {"bond_kekule", bond_kekule, n_bonds}, {"bond_aromatic", bond_aromatic, n_bonds},
        {"implicit_h", implicit_h, n_lig}, {"atom_flags", atom_flags, n_lig}, {"valence_status", valence_status, n_graphs},
        {"atom_terms", atom_terms, n_lig}, {"lig_type", lig_type, n_lig}, {"bond_rotatable", bond_rotatable, n_bonds},
        {"graph_terms", graph_terms, n_graphs}, {"graph_out", graph_out, n_graphs}};
    const int rc = device_visible("ligand_interactions", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_interactions(x_lig, z_lig, lig_ptr, n_lig, x_rec, rec_type, rec_ptr, n_rec, n_graphs, bond_ptr,
                                                    bond_index, bond_kekule, bond_aromatic, n_bonds, implicit_h, atom_flags,
                                                    valence_status, atom_terms, lig_type, bond_rotatable, graph_terms, graph_out,
                                                    (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_interactions: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_groups(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                       const int32_t* bond_index, const uint8_t* bond_order, const uint8_t* bond_aromatic, int n_bonds,
                       int32_t* atom_group, uint8_t* atom_class, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_groups: negative count (B=%d n_lig=%d n_bonds=%d)", n_graphs, n_lig, n_bonds);
    if ((n_graphs > 0 && (!lig_ptr || !bond_ptr || !graph_out)) || (n_lig > 0 && (!z_lig || !atom_group || !atom_class)) ||
        (n_bonds > 0 && (!bond_index || !bond_order)))
        return set_error(CBGX_E_INVALID, "ligand_groups: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const DeviceArray arrays[] = {
        {"z_lig", z_lig, n_lig}, {"lig_ptr", lig_ptr, n_graphs + 1}, {"bond_ptr", bond_ptr, n_lig + 1}, {"bond_index", bond_index, n_bonds},
        {"bond_order", bond_order, n_bonds}, {"bond_aromatic", bond_aromatic, n_bonds}, {"atom_group", atom_group, n_lig},
        {"atom_class", atom_class, n_lig}, {"graph_out", graph_out, n_graphs}};
    const int rc = device_visible("ligand_groups", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_groups(z_lig, lig_ptr, n_lig, n_graphs, bond_ptr, bond_index, bond_order, bond_aromatic, n_bonds,
                                              atom_group, atom_class, graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_groups: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_groups_templates(uint8_t* n_atoms, uint8_t* n_bonds, uint8_t* labels, uint8_t* bonds) {
    if (!n_atoms || !n_bonds || !labels || !bonds) return set_error(CBGX_E_INVALID, "ligand_groups_templates: NULL pointer");
    ligand_groups_templates(n_atoms, n_bonds, labels, bonds);
    return CBGX_OK;
}

int cbgx_ligand_fingerprints(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                             const int32_t* bond_index, const uint8_t* bond_type, const uint8_t* atom_ring_min, int n_bonds, uint32_t* fp,
                             uint64_t* mol_hash, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_bonds < 0)
        return set_error(CBGX_E_INVALID, "ligand_fingerprints: negative count (B=%d n_lig=%d n_bonds=%d)", n_graphs, n_lig, n_bonds);
    if ((n_graphs > 0 && (!lig_ptr || !bond_ptr || !fp || !mol_hash || !graph_out)) || (n_lig > 0 && (!z_lig || !atom_ring_min)) ||
        (n_bonds > 0 && (!bond_index || !bond_type)))
        return set_error(CBGX_E_INVALID, "ligand_fingerprints: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const DeviceArray arrays[] = {
        {"z_lig", z_lig, n_lig}, {"lig_ptr", lig_ptr, n_graphs + 1}, {"bond_ptr", bond_ptr, n_lig + 1}, {"bond_index", bond_index, n_bonds},
        {"bond_type", bond_type, n_bonds}, {"atom_ring_min", atom_ring_min, n_lig}, {"fp", fp, n_graphs}, {"mol_hash", mol_hash, n_graphs},
        {"graph_out", graph_out, n_graphs}};
    const int rc = device_visible("ligand_fingerprints", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_fingerprints(z_lig, lig_ptr, n_lig, n_graphs, bond_ptr, bond_index, bond_type, atom_ring_min, n_bonds,
                                                    fp, mol_hash, graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_fingerprints: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_group_diversity(const uint32_t* fp, const uint64_t* mol_hash, const int32_t* status, const int32_t* group_ptr,
                         const int64_t* pair_ptr, int n_graphs, int n_groups, long long n_pairs, int32_t* pair_sim, int32_t* first_same,
                         int32_t* nearest, int32_t* nearest_micro, int64_t* group_out, void* stream) {
    if (n_graphs < 0 || n_groups < 0 || n_pairs < 0)
        return set_error(CBGX_E_INVALID, "group_diversity: negative count (B=%d P=%d n_pairs=%lld)", n_graphs, n_groups, n_pairs);
    if ((n_groups > 0 && (!group_ptr || !pair_ptr || !group_out)) ||
        (n_graphs > 0 && (!fp || !mol_hash || !status || !first_same || !nearest || !nearest_micro)) || (n_pairs > 0 && !pair_sim))
        return set_error(CBGX_E_INVALID, "group_diversity: NULL pointer");
    if (n_groups == 0) return CBGX_OK;
    if ((uintptr_t)fp % 16 != 0) return set_error(CBGX_E_INVALID, "group_diversity: fp is not aligned to 16 bytes");
    const DeviceArray arrays[] = {
        {"fp", fp, n_graphs}, {"mol_hash", mol_hash, n_graphs}, {"status", status, n_graphs}, {"group_ptr", group_ptr, n_groups + 1},
        {"pair_ptr", pair_ptr, n_groups + 1}, {"pair_sim", pair_sim, n_pairs > 0 ? 1 : 0}, {"first_same", first_same, n_graphs},
        {"nearest", nearest, n_graphs}, {"nearest_micro", nearest_micro, n_graphs}, {"group_out", group_out, n_groups}};
    const int rc = device_visible("group_diversity", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_group_diversity(fp, mol_hash, status, group_ptr, pair_ptr, n_graphs, n_groups, n_pairs, pair_sim, first_same,
                                                nearest, nearest_micro, group_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "group_diversity: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_pocket_contacts(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                         const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, double cutoff2, uint8_t* rec_contact,
                         uint8_t* lig_contact, double* centroid, int32_t* graph_out, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_rec < 0)
        return set_error(CBGX_E_INVALID, "pocket_contacts: negative count (B=%d n_lig=%d n_rec=%d)", n_graphs, n_lig, n_rec);
    if ((n_graphs > 0 && (!lig_ptr || !rec_ptr || !centroid || !graph_out)) || (n_lig > 0 && (!x_lig || !z_lig || !lig_contact)) ||
        (n_rec > 0 && (!x_rec || !z_rec || !rec_contact)))
        return set_error(CBGX_E_INVALID, "pocket_contacts: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const DeviceArray arrays[] = {
        {"x_lig", x_lig, n_lig}, {"z_lig", z_lig, n_lig}, {"lig_ptr", lig_ptr, n_graphs + 1}, {"x_rec", x_rec, n_rec},
        {"z_rec", z_rec, n_rec}, {"rec_ptr", rec_ptr, n_graphs + 1}, {"rec_contact", rec_contact, n_rec},
        {"lig_contact", lig_contact, n_lig}, {"centroid", centroid, n_graphs}, {"graph_out", graph_out, n_graphs}};
    int rc = device_visible("pocket_contacts", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    rc = check_ligand_sizes("pocket_contacts", lig_ptr, n_lig, n_graphs, (hipStream_t)stream);
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_pocket_contacts(x_lig, z_lig, lig_ptr, n_lig, x_rec, z_rec, rec_ptr, n_rec, n_graphs, cutoff2, rec_contact,
                                                lig_contact, centroid, graph_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "pocket_contacts: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_native_compare(const uint32_t* fp, const uint64_t* mol_hash, const int32_t* fp_status, const uint8_t* rec_contact,
                        const int32_t* rec_ptr, const double* centroid, const int32_t* contacts_status, int n_graphs, int n_rec,
                        const uint32_t* fp_nat, const uint64_t* mol_hash_nat, const int32_t* fp_status_nat, const uint8_t* rec_contact_nat,
                        const int32_t* rec_ptr_nat, const double* centroid_nat, const int32_t* contacts_status_nat, int n_groups,
                        int n_rec_nat, const int32_t* group_ptr, int64_t* sample_out, double* centroid_d2, int64_t* group_out,
                        void* stream) {
    if (n_graphs < 0 || n_rec < 0 || n_groups < 0 || n_rec_nat < 0)
        return set_error(CBGX_E_INVALID, "native_compare: negative count (B=%d n_rec=%d P=%d n_rec_nat=%d)", n_graphs, n_rec, n_groups,
                         n_rec_nat);
    if ((n_graphs > 0 && (!fp || !mol_hash || !fp_status || !centroid || !contacts_status || !sample_out || !centroid_d2)) ||
        (n_rec > 0 && !rec_contact) ||
        (n_groups > 0 && (!rec_ptr || !fp_nat || !mol_hash_nat || !fp_status_nat || !rec_ptr_nat || !centroid_nat || !contacts_status_nat ||
                          !group_ptr || !group_out)) ||
        (n_rec_nat > 0 && !rec_contact_nat))
        return set_error(CBGX_E_INVALID, "native_compare: NULL pointer");
    if (n_groups == 0) return CBGX_OK;
    if ((uintptr_t)fp % 16 != 0 || (uintptr_t)fp_nat % 16 != 0)
        return set_error(CBGX_E_INVALID, "native_compare: %s is not aligned to 16 bytes", (uintptr_t)fp % 16 != 0 ? "fp" : "fp_nat");
    const DeviceArray arrays[] = {
        {"fp", fp, n_graphs}, {"mol_hash", mol_hash, n_graphs}, {"fp_status", fp_status, n_graphs}, {"rec_contact", rec_contact, n_rec},
        {"rec_ptr", rec_ptr, n_graphs + 1}, {"centroid", centroid, n_graphs}, {"contacts_status", contacts_status, n_graphs},
        {"fp_nat", fp_nat, n_groups}, {"mol_hash_nat", mol_hash_nat, n_groups}, {"fp_status_nat", fp_status_nat, n_groups},
        {"rec_contact_nat", rec_contact_nat, n_rec_nat}, {"rec_ptr_nat", rec_ptr_nat, n_groups + 1}, {"centroid_nat", centroid_nat, n_groups},
        {"contacts_status_nat", contacts_status_nat, n_groups}, {"group_ptr", group_ptr, n_groups + 1},
        {"sample_out", sample_out, n_graphs}, {"centroid_d2", centroid_d2, n_graphs}, {"group_out", group_out, n_groups}};
    const int rc = device_visible("native_compare", arrays, (int)(sizeof(arrays) / sizeof(arrays[0])));
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_native_compare(fp, mol_hash, fp_status, rec_contact, rec_ptr, centroid, contacts_status, n_graphs, n_rec, fp_nat,
                                               mol_hash_nat, fp_status_nat, rec_contact_nat, rec_ptr_nat, centroid_nat, contacts_status_nat,
                                               n_groups, n_rec_nat, group_ptr, sample_out, centroid_d2, group_out, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "native_compare: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_pair_hist(const float* x_lig,const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                          const double* edges_all, int n_edges_all, const double* edges_cc, int n_edges_cc, int32_t* pair_hist,
                          void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_edges_all < 0 || n_edges_cc < 0)
        return set_error(CBGX_E_INVALID, "ligand_pair_hist: negative count (B=%d n_lig=%d edges=%d, %d)", n_graphs, n_lig, n_edges_all,
                         n_edges_cc);
    if (n_edges_all > CBGX_PAIR_HIST_MAX_EDGES || n_edges_cc > CBGX_PAIR_HIST_MAX_EDGES)
        return set_error(CBGX_E_INVALID, "ligand_pair_hist: %d and %d edges, more than the %d a histogram row holds", n_edges_all,
                         n_edges_cc, CBGX_PAIR_HIST_MAX_EDGES);
    if ((n_graphs > 0 && (!lig_ptr || !pair_hist)) || (n_lig > 0 && (!x_lig || !z_lig)) || (n_edges_all > 0 && !edges_all) ||
        (n_edges_cc > 0 && !edges_cc))
        return set_error(CBGX_E_INVALID, "ligand_pair_hist: NULL pointer");
    if (n_graphs == 0) return CBGX_OK;
    const int rc = check_ligand_sizes("ligand_pair_hist", lig_ptr, n_lig, n_graphs, (hipStream_t)stream);
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_pair_hist(x_lig, z_lig, lig_ptr, n_lig, n_graphs, edges_all, n_edges_all, edges_cc, n_edges_cc,
                                                 pair_hist, (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_pair_hist: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_angles(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* adj_ptr,
                       const int32_t* adj_nbr, const uint8_t* adj_order, int n_adj, const int32_t* angle_ptr, int n_angles,
                       const double* cos_edges, int n_cos_edges, int32_t* angle_index, double* angle_cos, uint8_t* angle_bin,
                       int16_t* angle_type, void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_adj < 0 || n_angles < 0 || n_cos_edges < 0)
        return set_error(CBGX_E_INVALID, "ligand_angles: negative count (B=%d n_lig=%d n_adj=%d n_angles=%d edges=%d)", n_graphs, n_lig,
                         n_adj, n_angles, n_cos_edges);
    if (n_cos_edges > CBGX_ANGLES_MAX_EDGES)
        return set_error(CBGX_E_INVALID, "ligand_angles: %d edges, more than the %d a uint8 bin beside the degenerate mark holds",
                         n_cos_edges, CBGX_ANGLES_MAX_EDGES);
    if ((n_graphs > 0 && (!lig_ptr || !adj_ptr || !angle_ptr)) || (n_lig > 0 && (!x_lig || !z_lig)) ||
        (n_adj > 0 && (!adj_nbr || !adj_order)) || (n_angles > 0 && (!angle_index || !angle_cos || !angle_bin || !angle_type)) ||
        (n_cos_edges > 0 && !cos_edges))
        return set_error(CBGX_E_INVALID, "ligand_angles: NULL pointer");
    if (n_graphs == 0 || n_angles == 0) return CBGX_OK;
    const int rc = check_ligand_sizes("ligand_angles", lig_ptr, n_lig, n_graphs, (hipStream_t)stream);
    if (rc != CBGX_OK) return rc;
    const hipError_t e = launch_ligand_angles(x_lig, z_lig, lig_ptr, n_lig, n_graphs, adj_ptr, adj_nbr, adj_order, n_adj, angle_ptr,
                                              n_angles, cos_edges, n_cos_edges, angle_index, angle_cos, angle_bin, angle_type,
                                              (hipStream_t)stream);
    if (e != hipSuccess) return set_error(CBGX_E_HIP, "ligand_angles: launch: %s", hipGetErrorString(e));
    return CBGX_OK;
}

int cbgx_ligand_geometry_tables(int32_t* bond_pm, int32_t* margins, int32_t* allowed, uint8_t* elements, uint8_t* vdw_z, double* vdw_r,
                                double* tolerance) {
    ligand_geometry_tables(bond_pm, margins, allowed, elements, vdw_z, vdw_r, tolerance);
    return CBGX_OK;
}

}  // extern "C"

/*
 * assembly_classes.hpp -- what the degree-7 line stiffness kernel needs to complete rows of the boolean gather Qt
 * (points -> dofs) itself (flag "assemble_in_stiffness", fdd_stiffness_matrix_lines_direct): the class of every row of Qt,
 * read off Qt's own arrays and the element lists, with no assumption about the mesh (as detect_shared_blocks reads the
 * factor arrays).
 *
 *   single   the row has exactly one entry;
 *   pair     exactly two, in column order the point (7, j, k) of element e and the point (0, j, k) of element e + 1 of one
 *            3-D degree-7 list, same j and k, e / 4 == (e + 1) / 4: the two elements are waves of one workgroup of the
 *            line kernel (element = 4 * workgroup + wave);
 *   general  everything else.
 *
 * A row is never split: its points all carry the row's class (pair: low for the first entry, high for the second), and a
 * point that occurs in no row is a point without a dof.  From that: point_dof with the class in the two bits above
 * kDofBits, and the general rows as a CSR of their own -- renumbered, entries contiguous, columns still point indices, with
 * the row -> dof map -- so that its plan's row blocks are full ones.
 */
#ifndef FDD_ASSEMBLY_CLASSES_HPP
#define FDD_ASSEMBLY_CLASSES_HPP

#include <string>
#include <vector>

#include "element_operator.hpp"

namespace fdd
{

struct AssemblyClasses
{
    // the encoding fdd_stiffness_matrix_lines_direct reads (fdd_hip.h)
    static constexpr int kDofBits = 29;
    enum : int
    {
        general = 0,
        single = 1,
        pair_low = 2,
        pair_high = 3,
        none = 4 // in the counts only: such a point keeps its negative entry
    };

    bool built = false;
    std::string unusable;          // why the arrays below cannot be used whatever the flags say ("": they can)
    long long rows[3] = {0, 0, 0}; // general, single, pair
    long long points[5] = {0, 0, 0, 0, 0};
    int reduced_blocks = 0; // row blocks of the general rows' plan (known once it is made: ensure_device)
    std::vector<int> point_class_dof, ptr, col, row_map;

    // device copies and the plan of the general rows, made when first used
    bool on_device = false;
    memory point_class_dof_dev, ptr_dev, col_dev, row_map_dev;
    csr_plan plan;

    void clear()
    {
        *this = AssemblyClasses();
    }

    // Qt: num_rows rows over num_points columns, host arrays; point_dof: the dof of every point (negative: none), whose
    // non-negative entries are what Qt's columns say -- checked here, a disagreement makes the result unusable
    void build(const int *qt_ptr, const int *qt_col, int num_rows, int num_points, const std::vector<int> &point_dof, const std::vector<LevelList> &lists)
    {
        clear();
        built = true;
        point_class_dof.assign(point_dof.begin(), point_dof.end());
        std::vector<char> cls((size_t)num_rows, (char)general);
        // element and lattice position of a point of a 3-D degree-7 list; false: the point lies in no such list
        const auto locate = [&](int p, int &list, int &e, int &i, int &jk) {
            for (size_t t = 0; t < lists.size(); t++)
            {
                const LevelList &ll = lists[t];
                if (ll.dim != 3 or ll.poly_degree != 7 or p < ll.first_offset or (long long)p >= (long long)ll.first_offset + (long long)ll.num_points()) continue;
                const int at = p - ll.first_offset;
                list = (int)t, e = at / 512, i = at & 7, jk = (at >> 3) & 63;
                return true;
            }
            return false;
        };
        bool consistent = (int)point_dof.size() == num_points;
        std::vector<char> seen((size_t)num_points, 0);
        for (int r = 0; r < num_rows; r++)
        {
            const int len = qt_ptr[r + 1] - qt_ptr[r];
            const int *c = qt_col + qt_ptr[r];
            for (int t = 0; t < len; t++)
            {
                if (c[t] < 0 or c[t] >= num_points or (consistent and (point_dof[c[t]] != r or seen[c[t]])))
                    consistent = false;
                else
                    seen[c[t]] = 1;
            }
            if (len == 1)
                cls[r] = (char)single;
            else if (len == 2 and consistent)
            {
                int l0, e0, i0, jk0, l1, e1, i1, jk1;
                if (locate(c[0], l0, e0, i0, jk0) and locate(c[1], l1, e1, i1, jk1) and l0 == l1 and e1 == e0 + 1 and i0 == 7 and i1 == 0 and jk0 == jk1 and e0 / 4 == e1 / 4) cls[r] = (char)pair_low;
            }
        }
        if (consistent)
            for (int p = 0; p < num_points; p++)
                if ((point_dof[p] >= 0) != (seen[p] != 0)) consistent = false;
        if (not consistent)
            unusable = "point_dof is not the transpose of Qt's columns";
        else if (num_rows > (1 << kDofBits))
            unusable = "the dof count leaves no spare bits in point_dof";
        if (not unusable.empty())
        {
            point_class_dof.clear();
            return;
        }
        // the classes into the points, the general rows into their own CSR
        ptr.assign(1, 0);
        for (int r = 0; r < num_rows; r++)
        {
            const int len = qt_ptr[r + 1] - qt_ptr[r];
            const int *c = qt_col + qt_ptr[r];
            const int k = cls[r] == (char)pair_low ? 2 : (int)cls[r];
            rows[k]++; // a row without entries is a general row: the gather writes its T(0)
            for (int t = 0; t < len; t++)
            {
                const int pc = cls[r] == (char)pair_low ? (t == 0 ? pair_low : pair_high) : (int)cls[r];
                point_class_dof[c[t]] = r | (pc << kDofBits);
                points[pc]++;
            }
        }
        for (int r = 0; r < num_rows; r++)
            if (cls[r] == (char)general)
            {
                col.insert(col.end(), qt_col + qt_ptr[r], qt_col + qt_ptr[r + 1]);
                ptr.push_back((int)col.size());
                row_map.push_back(r);
            }
        points[none] = (long long)num_points - points[general] - points[single] - points[pair_low] - points[pair_high];
    }

    // false (with the reason in unusable): the general rows' plan does not run on the kernel that stores through a row map
    bool ensure_device()
    {
        if (on_device) return true;
        if (not built or not unusable.empty()) return false;
        const size_t nr = row_map.size();
        if (nr > 0)
        {
            plan = make_csr_plan(ptr.data(), (int)nr, (int)point_class_dof.size(), (int)col.size());
            FDD_CALL(fdd_csr_plan_set_unit_values(plan.get(), 1));
            int pipelined = 0;
            FDD_CALL(fdd_csr_plan_pipelined(plan.get(), &pipelined));
            FDD_CALL(fdd_csr_plan_num_blocks(plan.get(), &reduced_blocks));
            if (not pipelined)
            {
                plan.reset();
                unusable = "the plan of the general rows does not run on the pipelined short-row kernel";
                return false;
            }
            ptr_dev = dev().malloc<int>(nr + 1), col_dev = dev().malloc<int>(col.size()), row_map_dev = dev().malloc<int>(nr);
            ptr_dev.copyFrom(ptr.data(), (nr + 1) * sizeof(int));
            col_dev.copyFrom(col.data(), col.size() * sizeof(int));
            row_map_dev.copyFrom(row_map.data(), nr * sizeof(int));
        }
        point_class_dof_dev = dev().malloc<int>(std::max<size_t>(point_class_dof.size(), 1));
        if (not point_class_dof.empty()) point_class_dof_dev.copyFrom(point_class_dof.data(), point_class_dof.size() * sizeof(int));
        on_device = true;
        return true;
    }

    // y[row_map[r]] = the sum of q over general row r: with the kernel's own rows, every row of y once
    void gather_general(double *y, const double *q) const
    {
        if (row_map.empty()) return;
        // per row: pointer 4, row map 4, y 8; per entry: column 4, value 8; the last pointer
        ProfileScope prof("csr_short_pipelined_kernel<gather, mapped>", 16.0 * (double)row_map.size() + 12.0 * (double)col.size() + 4.0);
        FDD_CALL(fdd_csr_plan_gather_mapped(plan.get(), y, row_map_dev.as<int>(), ptr_dev.as<int>(), col_dev.as<int>(), q, dev().stream));
    }
};

} // namespace fdd

#endif

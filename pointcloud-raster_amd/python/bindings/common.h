// common.h -- shared helpers of the _pcr extension module.
#pragma once

#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "pcr/core/trees.h"
#include "pcr/core/types.h"

namespace py = pybind11;

// A failed Status surfaces in Python as RuntimeError(message), as in the reference module.
inline void raise_if_error(const pcr::Status& s) {
    if (!s.ok()) throw std::runtime_error(s.message);
}

// A TreeTable as a dict of NumPy arrays row, col, x, y, height, crown_cells: row k is the tree with id k + 1.
inline py::dict tree_table_dict(const pcr::TreeTable& t) {
    auto column = [](const auto& v) {
        using T = typename std::decay_t<decltype(v)>::value_type;
        py::array_t<T> a((py::ssize_t)v.size());
        if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
        return a;
    };
    py::dict d;
    d["row"] = column(t.row);
    d["col"] = column(t.col);
    d["x"] = column(t.x);
    d["y"] = column(t.y);
    d["height"] = column(t.height);
    d["crown_cells"] = column(t.crown_cells);
    return d;
}

void bind_core(py::module_& m);      // enums + value types + GridConfig + Grid + PointCloud
void bind_engine(py::module_& m);    // filter, glyph, reductions, pipeline
void bind_io(py::module_& m);        // I/O names kept for import compatibility (not part of this build)

// mi355_multivec_sys.rs — GENERATED from include/mi355_multivec.h by scripts/gen_rust_sys.py; do not edit by hand.
// Raw `extern "C"` bindings of the multivector entry points of libmi355_ann.so (multivector
// columns), beside mi355_sys.rs.  Checked against the header by tests/test_multivec_abi.py: identical function set,
// argument counts, struct field order, field offsets and sizes.
#![allow(non_camel_case_types, non_upper_case_globals, dead_code)]
use core::ffi::c_void;
use super::mi355_sys::{mi355_search_params};

// ---- constants (1)
pub const MI355_MULTIVEC_MAX_QVEC: u32 = 1024;

// ---- opaque handles
#[repr(C)]
pub struct mi355_multivec {
    _private: [u8; 0],
}

// ---- descriptors (plain old data, `struct_size` = size_of::<Self>() as u32)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct mi355_multivec_desc {
    pub struct_size: u32,
    pub dim: u32,
    pub n_rows: u64,
    pub n_vectors: u64,
    pub dtype: u32,
    pub mem: u32,
    pub vectors: *const c_void,
    pub offsets: *const u64,
    pub row_ids: *const u64,
    pub metric: u32,
    pub device: i32,
}

// ---- entry points (6); statuses as in mi355_sys.rs (status_to_error there)
#[link(name = "mi355_ann")]
extern "C" {
    pub fn mi355_multivec_open(desc: *const mi355_multivec_desc, out: *mut *mut mi355_multivec) -> i32;
    pub fn mi355_multivec_close(mv: *mut mi355_multivec) -> i32;
    pub fn mi355_multivec_set_stream(mv: *mut mi355_multivec, hip_stream: *mut c_void) -> i32;
    pub fn mi355_multivec_sync(mv: *mut mi355_multivec) -> i32;
    pub fn mi355_multivec_info(mv: *const mi355_multivec, out_rows: *mut u64, out_vectors: *mut u64) -> i32;
    pub fn mi355_multivec_search(mv: *mut mi355_multivec, queries: *const f32, n_queries: u32, n_qvec: u32, params: *const mi355_search_params, out_rowids: *mut u64, out_dist: *mut f32, out_counts: *mut u32) -> i32;
}

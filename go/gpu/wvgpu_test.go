//go:build rocm

package gpu

import (
	"encoding/binary"
	"testing"
	"unsafe"

	"github.com/weaviate/weaviate/adapters/repos/db/helpers"
)

// A non-nil, empty AllowList returns nothing (V/flat/index.go:423-427);
// a nil one searches every row.
func TestEmptyAllowListReturnsNothing(t *testing.T) {
	ctx, err := Open(0)
	if err != nil {
		t.Skip("no GPU:", err)
	}
	defer ctx.Close()
	const n, dims = 1000, 16
	x, err := ctx.NewCorpus(KindF32, MetricL2, dims, 0, n)
	if err != nil {
		t.Fatal(err)
	}
	defer x.Close()
	ids := make([]uint64, n)
	rows := make([]float32, n*dims)
	for i := range ids {
		ids[i] = uint64(i)
		for j := 0; j < dims; j++ {
			rows[i*dims+j] = float32((i*31+j*7)%97) / 97
		}
	}
	if err := x.Add(ids, rows); err != nil {
		t.Fatal(err)
	}
	q := rows[:dims]
	got, _, err := x.Search(q, 10, helpers.NewAllowList())
	if err != nil || len(got) != 0 {
		t.Fatalf("empty allow list: %v results, err %v", len(got), err)
	}
	got, d, err := x.Search(q, 10, nil)
	if err != nil || len(got) != 10 || got[0] != 0 || d[0] != 0 {
		t.Fatalf("nil allow list: %v %v %v", got, d, err)
	}
	got, _, err = x.Search(q, 10, helpers.NewAllowList(5, 7))
	if err != nil || len(got) != 2 {
		t.Fatalf("allow list {5, 7}: %v %v", got, err)
	}
}

// SearchDevicePipelinedFiltered gives every query the result of Search with
// its own AllowList: a list, an empty list and no list in one launch, through
// a window that begins at the corpus's first id.
func TestSearchDevicePipelinedFiltered(t *testing.T) {
	ctx, err := Open(0)
	if err != nil {
		t.Skip("no GPU:", err)
	}
	defer ctx.Close()
	const n, dims, nq, k = 1000, 128, 3, 5
	const idBase = 640
	x, err := ctx.NewCorpus(KindF32, MetricL2, dims, idBase, n)
	if err != nil {
		t.Fatal(err)
	}
	defer x.Close()
	ids := make([]uint64, n)
	rows := make([]float32, n*dims)
	for i := range ids {
		ids[i] = idBase + uint64(i)
		for j := 0; j < dims; j++ {
			rows[i*dims+j] = float32((i*31+j*7)%97) / 97
		}
	}
	if err := x.Add(ids, rows); err != nil {
		t.Fatal(err)
	}
	allows := []helpers.AllowList{helpers.NewAllowList(idBase+5, idBase+7, idBase+900), helpers.NewAllowList(), nil}
	const stride = (n + 63) / 64
	words, err := AllowWindow(allows, idBase, stride)
	if err != nil {
		t.Fatal(err)
	}
	alloc := func(bytes uint64) unsafe.Pointer {
		p, e := ctx.DeviceAlloc(bytes, true)
		if e != nil {
			t.Fatal(e)
		}
		return p
	}
	b := DeviceBuffers{Queries: alloc(4 * nq * dims), IDs: alloc(8 * nq * k), Dists: alloc(4 * nq * k),
		Counts: alloc(4 * nq), WsBytes: x.WorkspaceSize(nq, k)}
	b.Workspace = alloc(b.WsBytes)
	da := DeviceAllow{Words: alloc(8 * nq * stride), Bytes: 8 * nq * stride, Stride: stride, FirstID: idBase}
	for _, p := range []unsafe.Pointer{b.Queries, b.IDs, b.Dists, b.Counts, b.Workspace, da.Words} {
		defer ctx.DeviceFree(p)
	}
	if err := ctx.CopyToDevice(b.Queries, rows[:nq*dims], nil); err != nil {
		t.Fatal(err)
	}
	if err := ctx.CopyWordsToDevice(da.Words, words, nil); err != nil {
		t.Fatal(err)
	}
	if err := x.SearchDevicePipelinedFiltered(b, nq, k, da); err != nil {
		t.Fatal(err)
	}
	gotIDs := make([]byte, 8*nq*k)
	gotCounts := make([]byte, 4*nq)
	if err := ctx.CopyFromDevice(gotIDs, b.IDs, nil); err != nil {
		t.Fatal(err)
	}
	if err := ctx.CopyFromDevice(gotCounts, b.Counts, nil); err != nil {
		t.Fatal(err)
	}
	for q := 0; q < nq; q++ {
		want, _, err := x.Search(rows[q*dims:(q+1)*dims], k, allows[q])
		if err != nil {
			t.Fatal(err)
		}
		cnt := int(binary.LittleEndian.Uint32(gotCounts[4*q:]))
		if cnt != len(want) {
			t.Fatalf("query %d: %d results, Search gives %d", q, cnt, len(want))
		}
		for i := 0; i < k; i++ {
			id := binary.LittleEndian.Uint64(gotIDs[8*(q*k+i):])
			if i < cnt && id != want[i] {
				t.Fatalf("query %d result %d: id %d, Search gives %d", q, i, id, want[i])
			}
			if i >= cnt && id != ^uint64(0) {
				t.Fatalf("query %d padding %d: id %d", q, i, id)
			}
		}
	}
	da.FirstID = idBase + 1
	if err := x.SearchDevicePipelinedFiltered(b, nq, k, da); err == nil {
		t.Fatal("a window that does not begin at a multiple of 64 was accepted")
	}
	da.FirstID, da.Bytes = idBase, 8*nq*stride-8
	if err := x.SearchDevicePipelinedFiltered(b, nq, k, da); err == nil {
		t.Fatal("a window shorter than nq rows was accepted")
	}
}

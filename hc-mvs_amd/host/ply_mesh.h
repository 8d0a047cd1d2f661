/*
 * hc-mvs_amd/host/ply_mesh.h -- reader of a triangle mesh in a PLY file, for DensifyPointCloud --sample-mesh (the reference loads its
 * mesh through Mesh::LoadPLY, Mesh.cpp:1404-1510: vertices x y z, faces as a list vertex_indices / vertex_index, optionally a list
 * texcoord of 6 floats per face and a header line "comment TextureFile <name>"; a face that is not a triangle is an error there too).
 * ascii and binary_little_endian; properties the sampler has no use for (normals, colours, other elements) are skipped.  Plain C++,
 * nothing but the standard library: the whole file is read into memory and every read is checked against its end, so a truncated or
 * lying file gives an error message, never an out-of-bounds access or an allocation sized by a number the file merely claims.
 */
#ifndef HCMVS_PLY_MESH_H
#define HCMVS_PLY_MESH_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

namespace plymesh {

struct Mesh {
	std::vector<float> vertices;    // n * 3
	std::vector<uint32_t> faces;    // m * 3
	std::vector<float> texcoords;   // m * 6 or empty
	std::string textureFile;        // "comment TextureFile <name>" or empty
};

namespace detail {

enum Type { I8, U8, I16, U16, I32, U32, F32, F64, BAD };
inline Type type_of(const std::string& t) {
	static const struct { const char* name; Type type; } kTypes[] = {
		{"char", I8}, {"int8", I8}, {"uchar", U8}, {"uint8", U8}, {"short", I16}, {"int16", I16}, {"ushort", U16}, {"uint16", U16},
		{"int", I32}, {"int32", I32}, {"uint", U32}, {"uint32", U32}, {"float", F32}, {"float32", F32}, {"double", F64}, {"float64", F64}};
	for (const auto& k : kTypes) if (t == k.name) return k.type;
	return BAD;
}
inline size_t size_of(Type t) { static const size_t s[] = {1, 1, 2, 2, 4, 4, 4, 8, 0}; return s[t]; }

struct Property { std::string name; bool list = false; Type count = BAD, type = BAD; };
struct Element { std::string name; unsigned long long count = 0; std::vector<Property> props; };

struct Cursor {
	const char* p; const char* end; bool ascii;
	// one value of type t as a double (exact for every integer type and for float); false at the end of the data or on a malformed number
	bool value(Type t, double& v) {
		if (ascii) {
			while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) ++p;
			const char* q = p;
			while (q < end && !(*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n')) ++q;
			if (q == p || q - p > 63) return false;
			char tok[64];
			memcpy(tok, p, (size_t)(q - p)); tok[q - p] = '\0';
			char* stop = nullptr;
			v = strtod(tok, &stop);
			if (stop == tok || *stop != '\0') return false;
			if (t == F32) v = (double)(float)v;
			p = q;
			return true;
		}
		const size_t n = size_of(t);
		if ((size_t)(end - p) < n) return false;
		switch (t) {
			case I8: { int8_t x; memcpy(&x, p, 1); v = x; break; }
			case U8: { uint8_t x; memcpy(&x, p, 1); v = x; break; }
			case I16: { int16_t x; memcpy(&x, p, 2); v = x; break; }
			case U16: { uint16_t x; memcpy(&x, p, 2); v = x; break; }
			case I32: { int32_t x; memcpy(&x, p, 4); v = x; break; }
			case U32: { uint32_t x; memcpy(&x, p, 4); v = x; break; }
			case F32: { float x; memcpy(&x, p, 4); v = x; break; }
			case F64: { double x; memcpy(&x, p, 8); v = x; break; }
			default: return false;
		}
		p += n;
		return true;
	}
};

inline bool fail(std::string& err, const std::string& what) { err = what; return false; }

} // namespace detail

// the mesh in `data` (the bytes of a PLY file); false with a message in err
inline bool parse(const char* data, size_t size, Mesh& mesh, std::string& err) {
	using namespace detail;
	mesh = Mesh();
	const char* p = data; const char* const end = data + size;
	auto line = [&](std::string& ln) { // the next header line without its end-of-line; false at the end of the data
		if (p >= end) return false;
		const char* q = (const char*)memchr(p, '\n', (size_t)(end - p));
		const char* stop = q ? q : end;
		ln.assign(p, (size_t)(stop - p));
		while (!ln.empty() && (ln.back() == '\r' || ln.back() == ' ')) ln.pop_back();
		p = q ? q + 1 : end;
		return true;
	};
	auto words = [](const std::string& ln) {
		std::vector<std::string> w;
		size_t i = 0;
		while (i < ln.size()) {
			while (i < ln.size() && (ln[i] == ' ' || ln[i] == '\t')) ++i;
			size_t j = i;
			while (j < ln.size() && ln[j] != ' ' && ln[j] != '\t') ++j;
			if (j > i) w.push_back(ln.substr(i, j - i));
			i = j;
		}
		return w;
	};
	std::string ln;
	if (!line(ln) || ln != "ply") return fail(err, "not a PLY file");
	int format = -1; // 0 ascii, 1 binary_little_endian
	std::vector<Element> elements;
	bool ended = false;
	while (line(ln)) {
		const std::vector<std::string> w = words(ln);
		if (w.empty()) continue;
		if (w[0] == "end_header") { ended = true; break; }
		if (w[0] == "format") {
			if (w.size() >= 2 && w[1] == "ascii") format = 0;
			else if (w.size() >= 2 && w[1] == "binary_little_endian") format = 1;
			else return fail(err, "unsupported PLY format '" + (w.size() >= 2 ? w[1] : std::string()) + "' (ascii or binary_little_endian expected)");
		} else if (w[0] == "comment") {
			if (w.size() >= 3 && w[1] == "TextureFile") mesh.textureFile = ln.substr(ln.find(w[2], ln.find("TextureFile") + 11));
		} else if (w[0] == "element") {
			if (w.size() != 3) return fail(err, "malformed element line '" + ln + "'");
			char* stop = nullptr;
			Element e;
			e.name = w[1];
			e.count = strtoull(w[2].c_str(), &stop, 10);
			if (*stop != '\0' || w[2][0] == '-') return fail(err, "malformed element count '" + w[2] + "'");
			elements.push_back(e);
		} else if (w[0] == "property") {
			if (elements.empty()) return fail(err, "a property before the first element");
			Property pr;
			if (w.size() == 5 && w[1] == "list") { pr.list = true; pr.count = type_of(w[2]); pr.type = type_of(w[3]); pr.name = w[4]; }
			else if (w.size() == 3) { pr.type = type_of(w[1]); pr.name = w[2]; }
			else return fail(err, "malformed property line '" + ln + "'");
			if (pr.type == BAD || (pr.list && (pr.count == BAD || pr.count == F32 || pr.count == F64))) return fail(err, "unknown type in '" + ln + "'");
			elements.back().props.push_back(pr);
		} else if (w[0] != "obj_info") return fail(err, "unknown header line '" + ln + "'");
	}
	if (!ended) return fail(err, "the header has no end_header");
	if (format < 0) return fail(err, "the header has no format line");
	Cursor cur{p, end, format == 0};
	const size_t left = (size_t)(end - p);
	bool haveV = false, haveF = false;
	for (const Element& e : elements) {
		// every row of an element takes at least one byte per property (two in ascii, counting the separator): a count beyond that is a lie
		// (the refusal below is the quick one; the bound that sizes the reserve follows)
		if (e.props.empty()) continue;
		if (e.count > left) return fail(err, "element " + e.name + " claims more rows than the file holds");
		// what is reserved ahead is bounded by the rows the bytes left can hold at the smallest size of a row
		size_t minRow = 0;
		for (const Property& pr : e.props) minRow += format == 0 ? 2 : size_of(pr.list ? pr.count : pr.type);
		const size_t rowsAhead = std::min<unsigned long long>(e.count, left / minRow);
		const bool isV = e.name == "vertex", isF = e.name == "face";
		int ix[3] = {-1, -1, -1}, iIdx = -1, iTex = -1;
		for (size_t k = 0; k < e.props.size(); ++k) {
			const Property& pr = e.props[k];
			if (isV && !pr.list) { if (pr.name == "x") ix[0] = (int)k; else if (pr.name == "y") ix[1] = (int)k; else if (pr.name == "z") ix[2] = (int)k; }
			if (isF && pr.list) { if (pr.name == "vertex_indices" || pr.name == "vertex_index") iIdx = (int)k; else if (pr.name == "texcoord") iTex = (int)k; }
		}
		if (isV) {
			if (ix[0] < 0 || ix[1] < 0 || ix[2] < 0) return fail(err, "the vertex element has no x, y, z");
			if (e.count > 0xFFFFFFFFull) return fail(err, "more than 2^32 - 1 vertices");
			haveV = true;
			mesh.vertices.reserve(rowsAhead * 3);
		}
		if (isF) {
			if (!haveV) return fail(err, "the face element comes before the vertex element");
			if (iIdx < 0) return fail(err, "the face element has no vertex_indices list");
			if (e.count > 0xFFFFFFFFull) return fail(err, "more than 2^32 - 1 faces");
			haveF = true;
			mesh.faces.reserve(rowsAhead * 3);
			if (iTex >= 0) mesh.texcoords.reserve(rowsAhead * 6);
		}
		const size_t nVerts = mesh.vertices.size() / 3;
		for (unsigned long long r = 0; r < e.count; ++r) {
			float xyz[3] = {0, 0, 0};
			for (size_t k = 0; k < e.props.size(); ++k) {
				const Property& pr = e.props[k];
				double v = 0;
				if (!pr.list) {
					if (!cur.value(pr.type, v)) return fail(err, "the file ends inside element " + e.name + " (row " + std::to_string(r) + ")");
					if (isV) for (int q = 0; q < 3; ++q) if (ix[q] == (int)k) xyz[q] = (float)v;
					continue;
				}
				double cnt = 0;
				if (!cur.value(pr.count, cnt)) return fail(err, "the file ends inside element " + e.name + " (row " + std::to_string(r) + ")");
				if (!(cnt >= 0) || cnt > 4294967295.0 || cnt != (double)(unsigned long long)cnt) return fail(err, "malformed list length in element " + e.name + " (row " + std::to_string(r) + ")");
				const unsigned long long n = (unsigned long long)cnt;
				if (isF && (int)k == iIdx && n != 3) return fail(err, "face " + std::to_string(r) + " has " + std::to_string(n) + " vertices: only triangles are supported");
				if (isF && (int)k == iTex && n != 6) return fail(err, "face " + std::to_string(r) + " has " + std::to_string(n) + " texture coordinates, 6 expected");
				for (unsigned long long j = 0; j < n; ++j) {
					if (!cur.value(pr.type, v)) return fail(err, "the file ends inside element " + e.name + " (row " + std::to_string(r) + ")");
					if (isF && (int)k == iIdx) {
						if (!(v >= 0) || v >= (double)nVerts || v != (double)(unsigned long long)v)
							return fail(err, "face " + std::to_string(r) + " names vertex " + std::to_string((long long)(v >= -9e18 && v <= 9e18 ? v : -1)) + " of " + std::to_string(nVerts));
						mesh.faces.push_back((uint32_t)v);
					} else if (isF && (int)k == iTex) mesh.texcoords.push_back((float)v);
				}
			}
			if (isV) mesh.vertices.insert(mesh.vertices.end(), xyz, xyz + 3);
		}
	}
	if (!haveV) return fail(err, "the file has no vertex element");
	if (!haveF) return fail(err, "the file has no face element");
	return true;
}

inline bool load(const std::string& path, Mesh& mesh, std::string& err) {
	std::ifstream f(path, std::ios::binary);
	if (!f) return detail::fail(err, "can not open the file");
	std::vector<char> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
	return parse(data.data(), data.size(), mesh, err);
}

} // namespace plymesh
#endif

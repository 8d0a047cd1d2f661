// tests/ply_mesh_shim.cpp -- the driver's PLY mesh reader (hc-mvs_amd/host/ply_mesh.h) as a stand-alone program, for
// tests/test_ply_mesh_parser.py: built with -fsanitize=address,undefined and run on good and on broken files.
// usage: ply_mesh_shim <file.ply>  ->  "ok <vertices> <faces> <texcoords> <checksum> [<texture file>]" and exit 0, or "error: <why>" and exit 1
#include "../hc-mvs_amd/host/ply_mesh.h"

#include <cstdio>

int main(int argc, char** argv) {
	if (argc != 2) { fprintf(stderr, "usage: ply_mesh_shim <file.ply>\n"); return 2; }
	plymesh::Mesh mesh;
	std::string err;
	if (!plymesh::load(argv[1], mesh, err)) { printf("error: %s\n", err.c_str()); return 1; }
	// touch everything that was read: a checksum over the vertices (as bits), the indices and the texture coordinates
	unsigned long long sum = 0;
	for (float v : mesh.vertices) { uint32_t b; memcpy(&b, &v, 4); sum = sum * 1099511628211ull + b; }
	for (uint32_t i : mesh.faces) sum = sum * 1099511628211ull + i;
	for (float v : mesh.texcoords) { uint32_t b; memcpy(&b, &v, 4); sum = sum * 1099511628211ull + b; }
	printf("ok %zu %zu %zu %llu %s\n", mesh.vertices.size() / 3, mesh.faces.size() / 3, mesh.texcoords.size() / 6, sum, mesh.textureFile.c_str());
	return 0;
}

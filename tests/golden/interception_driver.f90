!  interception_driver.f90 -- TEST INFRASTRUCTURE, not product code.
!
!  A bind(C) driver over the UNMODIFIED reference module mw_interception_store, compiled by tests/golden/make_interception.py
!  against the module files and objects the oracle recipe leaves in oracle/_ref/obj_parity (same flags: -O2 -ffp-contract=off).
!  It fills SetupDT / MeshDT / Input_DataDT from flat arrays the way oracle/ref/ref_capi.f90 does, calls the reference's
!  adjust_interception_store (smash/solver/routine/mw_interception_store.f90:19-160) and hands parameters%ci back.
!
!  This file is ours; it contains no reference source text.  Nothing compiled from it is committed.

module interception_driver

    use iso_c_binding
    use md_constant
    use mwd_setup
    use mwd_mesh
    use mwd_input_data
    use mwd_parameters
    use mw_sparse_storage
    use mw_interception_store, only: adjust_interception_store

    implicit none

contains

    !  icfg = (structure id: 2 gr-b, 3 gr-c; nrow; ncol; nt; sparse_storage 0/1; nday; nrep)
    !  arrays column-major as the reference holds them, path 1-based; ci is inout: the routine writes active cells only
    !  elapsed: seconds of the fastest of nrep calls of the routine alone (the set-up is not timed)
    subroutine ici_run(icfg, dt, path, active_cell, prcp, pet, day_index, ci, elapsed) bind(C, name="ici_run")

        integer(c_int), intent(in) :: icfg(7)
        real(c_float), intent(in) :: dt
        integer(c_int), intent(in) :: path(2, icfg(2)*icfg(3)), active_cell(icfg(2), icfg(3))
        real(c_float), intent(in) :: prcp(icfg(2), icfg(3), icfg(4)), pet(icfg(2), icfg(3), icfg(4))
        integer(c_int), intent(in) :: day_index(icfg(4))
        real(c_float), intent(inout) :: ci(icfg(2), icfg(3))
        real(c_double), intent(inout) :: elapsed

        type(SetupDT) :: setup
        type(MeshDT) :: mesh
        type(Input_DataDT) :: input_data
        type(ParametersDT) :: p
        integer :: nrow, ncol, nt, t, rep
        integer(8) :: c0, c1, crate
        real(c_double) :: one

        nrow = icfg(2); ncol = icfg(3); nt = icfg(4)
        if (icfg(1) .eq. 3) then
            setup%structure = "gr-c"
        else
            setup%structure = "gr-b"
        end if
        setup%dt = dt
        setup%sparse_storage = (icfg(5) .ne. 0)
        setup%ntime_step = nt
        call SetupDT_initialise(setup, 0, 0)

        call MeshDT_initialise(mesh, setup, nrow, ncol, 0)
        mesh%path = path
        mesh%active_cell = active_cell
        mesh%nac = count(active_cell .eq. 1)
        if (setup%sparse_storage) call compute_rowcol_to_ind_sparse(mesh)

        call Input_DataDT_initialise(input_data, setup, mesh)
        if (setup%sparse_storage) then
            do t = 1, nt
                call sparse_matrix_to_vector_r(mesh, prcp(:, :, t), input_data%sparse_prcp(:, t))
                call sparse_matrix_to_vector_r(mesh, pet(:, :, t), input_data%sparse_pet(:, t))
            end do
        else
            input_data%prcp = prcp
            input_data%pet = pet
        end if

        call ParametersDT_initialise(p, mesh)
        elapsed = huge(1._c_double)
        do rep = 1, max(1, icfg(7))
            p%ci = ci
            call system_clock(c0, crate)
            call adjust_interception_store(setup, mesh, input_data, p, icfg(6), day_index)
            call system_clock(c1)
            one = real(c1 - c0, c_double)/real(crate, c_double)
            if (one .lt. elapsed) elapsed = one
        end do
        ci = p%ci

    end subroutine ici_run

end module interception_driver
